/*
 * nfc_record.hip - device kernels of nfcgpu_record: float samples to int16 PCM and the receiver's levels in one pass.
 * The arithmetic is nfc_record.hpp; this file adds the grid, the loads and stores and the reductions' plumbing.
 *
 * nfc_record_kernel_*: a workgroup (4 waves) per segment of 16 384 samples of one buffer, segments x buffers in one grid. A lane
 * reads its quad of samples with 16-byte loads (one for mono, two for I/Q: input rows are aligned to a sample only, which a
 * dword-aligned global load does not mind) and writes PCM in aligned words of four samples: 8 bytes mono, 16 bytes I/Q. A
 * row that does not start on a word boundary (a mono row may start on any 2-byte boundary) has its words straddle two quads: a
 * word is then put together from the lane's own quad and its left neighbour's (a shuffle; lane 0 takes lane 63's of the step
 * before, and at the start of a wave's run converts the quad before it once more - 16 or 32 bytes in 64 KiB read twice, and only
 * for such rows). Element stores are left for the few samples before a row's first and behind its last whole word. Stride,
 * mode and levels are template parameters; the row's misalignment is uniform over the workgroup.
 *
 * Levels: registers, a butterfly over the wave, the four waves through LDS, one partial per segment to the context's scratch;
 * nfc_record_finish_kernel, a wave per buffer, combines a buffer's partials in index order. No atomics: the order of every
 * sum is fixed by sample index.
 */
#include <hip/hip_runtime.h>

#include "nfc_record.hpp"

namespace {

template <int CH>
__device__ __forceinline__ void nfc_record_store_word(uint8_t *at, const uint32_t e[4])
{
   if (CH == 1)
   {
      uint2 w;
      w.x = e[0] | (e[1] << 16);
      w.y = e[2] | (e[3] << 16);
      *reinterpret_cast<uint2 *>(at) = w;
   }
   else
   {
      uint4 w;
      w.x = e[0];
      w.y = e[1];
      w.z = e[2];
      w.w = e[3];
      *reinterpret_cast<uint4 *>(at) = w;
   }
}

template <int CH>
__device__ __forceinline__ void nfc_record_store_element(uint8_t *at, uint32_t e)
{
   if (CH == 1)
      *reinterpret_cast<uint16_t *>(at) = (uint16_t)e;
   else
      *reinterpret_cast<uint32_t *>(at) = e;
}

__device__ __forceinline__ NfcRecordPartial nfc_record_wave_sum(NfcRecordPartial acc)
{
   for (int off = 1; off < 64; off <<= 1)
   {
      NfcRecordPartial other;
      other.power = __shfl_xor(acc.power, off);
      other.average = __shfl_xor(acc.average, off);
      other.peak = __shfl_xor(acc.peak, off);
      other.clipped = __shfl_xor(acc.clipped, off);
      acc = nfc_record_add(acc, other);
   }
   return acc;
}

__device__ __forceinline__ float nfc_record_wave_sum(float v)
{
   for (int off = 1; off < 64; off <<= 1)
      v = v + __shfl_xor(v, off);
   return v;
}

template <int STRIDE, int MODE, bool LEVELS>
__device__ __forceinline__ void nfc_record_block(const NfcRecordArgs &A)
{
   constexpr int CH = NfcRecordKind<STRIDE, MODE>::kChannels;
   constexpr uint32_t EB = 2 * CH;          /* bytes of a PCM sample */
   constexpr uint32_t IB = 4 * STRIDE;      /* bytes of an input sample */

   __shared__ NfcRecordPartial waves[NfcRecordShape::kWaves];

   const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
   const uint32_t n = A.n;

   for (uint64_t item = blockIdx.x; item < A.total; item += gridDim.x)
   {
      const uint64_t b = item / A.nSegments;
      const uint32_t s = (uint32_t)(item % A.nSegments);
      const uint8_t *row = reinterpret_cast<const uint8_t *>(A.in) + b * A.inPitch;
      uint8_t *orow = reinterpret_cast<uint8_t *>(A.out) + b * A.outPitch;

      /* samples the row lies behind a word boundary: word W of the row, at base + W * 4 * EB, holds samples 4 W - a ... 4 W - a + 3 */
      const uint32_t a = (uint32_t)((reinterpret_cast<uintptr_t>(orow) & (4 * EB - 1)) / EB);
      uint8_t *base = orow - a * EB;
      const uint64_t wordsEnd = ((uint64_t)n + a) / 4;  /* whole words: W from (a ? 1 : 0) to here */

      const uint32_t q0 = s * NfcRecordShape::kSegmentQuads + wave * NfcRecordShape::kWaveQuads;

      NfcRecordPartial acc;
      nfc_record_begin(acc);

      if ((uint64_t)q0 * 4 < n)
      {
         uint32_t carry[4] = {0, 0, 0, 0};

         if (a)
         {
            /* the quad before the wave's run, for the word that straddles the two (it is whole whenever that word is) */
            if (lane == 0 && q0 > 0 && (uint64_t)q0 * 4 <= n)
            {
               NfcRecordPartial none;
               nfc_record_quad<STRIDE, MODE, false>(reinterpret_cast<const float *>(row + (uint64_t)(q0 - 1) * 4 * IB), 4, carry, none, A.w);
            }
            for (int p = 0; p < 4; p++)
               carry[p] = __shfl(carry[p], 0);
         }

#pragma unroll 2
         for (uint32_t t = 0; t < NfcRecordShape::kIters; t++)
         {
            const uint32_t q = q0 + t * 64 + lane;
            const uint64_t i0 = (uint64_t)q * 4;
            const uint32_t valid = i0 < n ? (n - i0 < 4 ? (uint32_t)(n - i0) : 4u) : 0u;
            uint32_t e[4] = {0, 0, 0, 0};

            if (valid)
               nfc_record_quad<STRIDE, MODE, LEVELS>(reinterpret_cast<const float *>(row + i0 * IB), valid, e, acc, A.w);
            else if (LEVELS)
               nfc_record_quad_none(acc, A.w);

            if (a == 0)
            {
               if (valid == 4)
                  nfc_record_store_word<CH>(base + i0 * EB, e);
               else
               {
                  for (uint32_t p = 0; p < valid; p++)
                     nfc_record_store_element<CH>(orow + (i0 + p) * EB, e[p]);
               }
            }
            else
            {
               uint32_t prev[4], w[4];

               for (int p = 0; p < 4; p++)
               {
                  const uint32_t left = __shfl_up(e[p], 1), end = __shfl(e[p], 63);
                  prev[p] = lane == 0 ? carry[p] : left;
                  carry[p] = end;
               }

               switch (a)
               {
                  case 1: w[0] = prev[3]; w[1] = e[0]; w[2] = e[1]; w[3] = e[2]; break;
                  case 2: w[0] = prev[2]; w[1] = prev[3]; w[2] = e[0]; w[3] = e[1]; break;
                  default: w[0] = prev[1]; w[1] = prev[2]; w[2] = prev[3]; w[3] = e[0]; break;
               }

               if (q >= 1 && q < wordsEnd)
                  nfc_record_store_word<CH>(base + i0 * EB, w);

               /* the samples no whole word holds: before word 1, behind the last */
               if (valid && (q == 0 || (uint64_t)q + 1 >= wordsEnd))
               {
                  for (uint32_t p = 0; p < valid; p++)
                  {
                     const uint64_t word = (i0 + p + a) / 4;
                     if (word < 1 || word >= wordsEnd)
                        nfc_record_store_element<CH>(orow + (i0 + p) * EB, e[p]);
                  }
               }
            }
         }
      }

      if (LEVELS)
      {
         nfc_record_lane_end(acc, lane, A.w);
         acc = nfc_record_wave_sum(acc);

         if (lane == 0)
            waves[wave] = acc;
         __syncthreads();

         if (threadIdx.x == 0)
            A.partials[item] = nfc_record_segment(waves, A.w);
         __syncthreads();
      }
   }
}

}

#define NFC_RECORD_KERNEL(name, STRIDE, MODE, LEVELS) \
   __global__ __launch_bounds__(NfcRecordShape::kThreads) void name(NfcRecordArgs A) { nfc_record_block<STRIDE, MODE, LEVELS>(A); }

NFC_RECORD_KERNEL(nfc_record_kernel_mono, 1, NFC_RECORD_SAME, false)
NFC_RECORD_KERNEL(nfc_record_kernel_mono_levels, 1, NFC_RECORD_SAME, true)
NFC_RECORD_KERNEL(nfc_record_kernel_iq, 2, NFC_RECORD_SAME, false)
NFC_RECORD_KERNEL(nfc_record_kernel_iq_levels, 2, NFC_RECORD_SAME, true)
NFC_RECORD_KERNEL(nfc_record_kernel_magnitude, 2, NFC_RECORD_MAGNITUDE, false)
NFC_RECORD_KERNEL(nfc_record_kernel_magnitude_levels, 2, NFC_RECORD_MAGNITUDE, true)

/* a wave per buffer: the buffer's segment partials, in index order, to its levels */
__global__ __launch_bounds__(64) void nfc_record_finish_kernel(NfcRecordArgs A)
{
   __shared__ float level1[4096]; /* sums of 64 segments each: 2^32 samples are 2^18 segments */
   __shared__ float level2[64];

   const uint32_t lane = threadIdx.x;
   const uint32_t m = A.nSegments;

   for (uint32_t b = blockIdx.x; b < A.nBuffers; b += gridDim.x)
   {
      const NfcRecordPartial *seg = A.partials + (uint64_t)b * m;

      float peak = nfc_record_nan();
      uint32_t clipped = 0;

      for (uint32_t s = lane; s < m; s += 64)
      {
         peak = nfc_record_max(peak, seg[s].peak);
         clipped += seg[s].clipped;
      }

      for (int off = 1; off < 64; off <<= 1)
      {
         peak = nfc_record_max(peak, __shfl_xor(peak, off));
         clipped += __shfl_xor(clipped, off);
      }

      /* power: groups of 64 until one value is left, short groups filled with zeros */
      float power;

      if (m == 1)
         power = seg[0].power;
      else
      {
         const uint32_t m1 = (m + 63) / 64;

         for (uint32_t g = 0; g < m1; g++)
         {
            const uint32_t at = g * 64 + lane;
            const float v = nfc_record_wave_sum(at < m ? seg[at].power : 0.0f);
            if (lane == 0)
               level1[g] = v;
         }
         __syncthreads();

         if (m1 == 1)
            power = level1[0];
         else
         {
            const uint32_t m2 = (m1 + 63) / 64;

            for (uint32_t g = 0; g < m2; g++)
            {
               const uint32_t at = g * 64 + lane;
               const float v = nfc_record_wave_sum(at < m1 ? level1[at] : 0.0f);
               if (lane == 0)
                  level2[g] = v;
            }
            __syncthreads();

            power = m2 == 1 ? level2[0] : nfc_record_wave_sum(lane < m2 ? level2[lane] : 0.0f);
         }
      }

      if (lane == 0)
         A.levels[b] = nfc_record_levels(power, nfc_record_chain_average(seg, m, A.w), peak, clipped, A.n);
      __syncthreads();
   }
}
