/*
 * nfc_spectrum.hip - device kernels of nfcgpu_spectrum: one workgroup per frame, every frame of every buffer in one launch.
 * The arithmetic is nfc_spectrum.hpp; this file adds the grid, the LDS and the barriers between the steps. Every length exists for
 * float I/Q and for int16 I/Q (nfcgpu_spectrum_fmt); the host picks.
 */
#include <hip/hip_runtime.h>

#include "nfc_spectrum.hpp"

namespace {

template <int L, int STEP, bool I16>
__device__ __forceinline__ void nfc_spectrum_steps(const NfcSpectrumArgs &A, uint64_t frame, int lane, NfcSpectrumRegs<L> &regs, float *ldsRe,
                                                   float *ldsIm)
{
   nfc_spectrum_step<L, STEP, I16>(A, frame, lane, regs, ldsRe, ldsIm);

   /* (the barrier after the last gather also keeps the next frame's first scatter behind it) */
   __syncthreads();

   if constexpr (STEP + 1 < NfcSpectrumShape<L>::kSteps)
      nfc_spectrum_steps<L, STEP + 1, I16>(A, frame, lane, regs, ldsRe, ldsIm);
}

template <int L, bool I16>
__device__ __forceinline__ void nfc_spectrum_block(const NfcSpectrumArgs &A)
{
   __shared__ float ldsRe[NfcSpectrumShape<L>::kLdsFloats];
   __shared__ float ldsIm[NfcSpectrumShape<L>::kLdsFloats];

   NfcSpectrumRegs<L> regs;

   for (uint64_t frame = blockIdx.x; frame < A.total; frame += gridDim.x)
      nfc_spectrum_steps<L, 0, I16>(A, frame, (int)threadIdx.x, regs, ldsRe, ldsIm);
}

}

/* Once per input format (nfc_sample.hpp), as the wave decoder and the envelope kernel: this text compiled a second time with
 * -DNFC_INPUT_I16 gives the kernels for the int16 pairs of a capture file (nfc_spectrum_kernel_i16_<L>), in an object of their
 * own, so that the float ones are the code they were. */
#ifdef NFC_INPUT_I16
#define NFC_SPECTRUM_KERNEL(L) \
   __global__ __launch_bounds__(NfcSpectrumShape<L>::kThreads) void nfc_spectrum_kernel_i16_##L(NfcSpectrumArgs A) { nfc_spectrum_block<L, true>(A); }
#else
#define NFC_SPECTRUM_KERNEL(L) \
   __global__ __launch_bounds__(NfcSpectrumShape<L>::kThreads) void nfc_spectrum_kernel_##L(NfcSpectrumArgs A) { nfc_spectrum_block<L, false>(A); }
#endif

NFC_SPECTRUM_KERNEL(256)
NFC_SPECTRUM_KERNEL(512)
NFC_SPECTRUM_KERNEL(1024)
NFC_SPECTRUM_KERNEL(2048)
NFC_SPECTRUM_KERNEL(4096)
