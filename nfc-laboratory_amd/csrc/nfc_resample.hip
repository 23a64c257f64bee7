/*
 * nfc_resample.hip - device kernels of nfcgpu_resample_radio_fmt for int16 magnitude, int16 I/Q and float I/Q rows: one lane per
 * buffer, 64 buffers per workgroup. What a lane does is nfc_resample.hpp; this file adds the grid, the ring in LDS, the staging and
 * the barriers. (Float magnitude rows are nfc_resample_radio_kernel of nfc_kernels.hip, as they were.)
 *
 * Staging. A tile is 32 samples of each of the 64 rows. A load instruction takes the tile's samples of two rows, a half wave per
 * row and a lane per sample - 64 B of an int16 magnitude row (16-bit loads: such a row may start on any 2-byte boundary), 128 B of
 * int16 I/Q (one 32-bit load per pair), 256 B of float I/Q (one 64-bit load). The 32 loads of a tile have no branch around them
 * (nfc_resample_fetch), so they are issued together, and they are issued one tile ahead: the wave asks for tile t + 1 once it has
 * parked tile t in the ring and decides tile t while those loads are on their way - a wave is alone on its SIMD here (64 buffers
 * per workgroup), so nobody else hides that latency. A value is converted, or its magnitude taken, when it is parked: the ring
 * holds floats, 32 consecutive ones per half wave and store. Measured: profiles/display_fmt.json, DESIGN.md section 6.
 */
#include <hip/hip_runtime.h>

#include "nfc_resample.hpp"

namespace {

template <uint32_t LAYOUT>
__device__ __forceinline__ void nfc_resample_block(const NfcResampleArgs &A)
{
   using S = NfcResampleShape;

   __shared__ float ring[S::kLanes * S::kPitch];

   const uint32_t lane = threadIdx.x;
   const uint32_t first = blockIdx.x * S::kLanes;
   const uint32_t buffer = first + lane;
   const bool mine = buffer < A.nBuffers;

   const float *window = ring + lane * S::kPitch;

   NfcResampleLane s;
   nfc_resample_begin(s);

   const uint32_t col = lane % S::kTile;
   const uint32_t half = lane / S::kTile;

   /* the lane's share of the tile on its way: sample col of rows half, 2 + half, ... */
   typename NfcResampleRaw<LAYOUT>::Type raw[S::kLanes / 2];

#pragma unroll
   for (uint32_t j = 0; j < S::kLanes / 2; j++)
      raw[j] = nfc_resample_fetch<LAYOUT>(A, first + 2 * j + half, col);

   for (uint32_t base = 0; base < A.n; base += S::kTile)
   {
      const uint32_t at = (base % S::kRing) + col;

#pragma unroll
      for (uint32_t j = 0; j < S::kLanes / 2; j++)
         ring[(2 * j + half) * S::kPitch + at] = nfc_resample_settle<LAYOUT>(A, first + 2 * j + half, base + col, raw[j]);

      __syncthreads();

      if (base + S::kTile < A.n)
      {
#pragma unroll
         for (uint32_t j = 0; j < S::kLanes / 2; j++)
            raw[j] = nfc_resample_fetch<LAYOUT>(A, first + 2 * j + half, base + S::kTile + col);
      }

      nfc_resample_decide(A, buffer, mine, s, window, base);

      __syncthreads();
   }

   nfc_resample_end(A, buffer, mine, s);
}

}

#define NFC_RESAMPLE_KERNEL(name, LAYOUT) \
   __global__ __launch_bounds__(64) void name(NfcResampleArgs A) { nfc_resample_block<LAYOUT>(A); }

NFC_RESAMPLE_KERNEL(nfc_resample_radio_kernel_i16, NFC_SAMPLE_I16 | 1u)
NFC_RESAMPLE_KERNEL(nfc_resample_radio_kernel_iq_i16, NFC_SAMPLE_I16 | 2u)
NFC_RESAMPLE_KERNEL(nfc_resample_radio_kernel_iq, 2u)
