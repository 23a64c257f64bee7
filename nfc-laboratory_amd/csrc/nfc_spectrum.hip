/*
 * nfc_spectrum.hip - device kernels of nfcgpu_spectrum: one workgroup per frame, every frame of every buffer in one launch.
 * The arithmetic is nfc_spectrum.hpp; this file adds the grid, the LDS and the barriers between the steps.
 */
#include <hip/hip_runtime.h>

#include "nfc_spectrum.hpp"

namespace {

template <int L, int STEP>
__device__ __forceinline__ void nfc_spectrum_steps(const NfcSpectrumArgs &A, uint64_t frame, int lane, NfcSpectrumRegs<L> &regs, float *ldsRe,
                                                   float *ldsIm)
{
   nfc_spectrum_step<L, STEP>(A, frame, lane, regs, ldsRe, ldsIm);

   /* (the barrier after the last gather also keeps the next frame's first scatter behind it) */
   __syncthreads();

   if constexpr (STEP + 1 < NfcSpectrumShape<L>::kSteps)
      nfc_spectrum_steps<L, STEP + 1>(A, frame, lane, regs, ldsRe, ldsIm);
}

template <int L>
__device__ __forceinline__ void nfc_spectrum_block(const NfcSpectrumArgs &A)
{
   __shared__ float ldsRe[NfcSpectrumShape<L>::kLdsFloats];
   __shared__ float ldsIm[NfcSpectrumShape<L>::kLdsFloats];

   NfcSpectrumRegs<L> regs;

   for (uint64_t frame = blockIdx.x; frame < A.total; frame += gridDim.x)
      nfc_spectrum_steps<L, 0>(A, frame, (int)threadIdx.x, regs, ldsRe, ldsIm);
}

}

#define NFC_SPECTRUM_KERNEL(L) \
   __global__ __launch_bounds__(NfcSpectrumShape<L>::kThreads) void nfc_spectrum_kernel_##L(NfcSpectrumArgs A) { nfc_spectrum_block<L>(A); }

NFC_SPECTRUM_KERNEL(256)
NFC_SPECTRUM_KERNEL(512)
NFC_SPECTRUM_KERNEL(1024)
NFC_SPECTRUM_KERNEL(2048)
NFC_SPECTRUM_KERNEL(4096)
