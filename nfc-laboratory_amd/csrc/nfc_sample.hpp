/*
 * nfc_sample.hpp - how the bytes of a submission become a magnitude, held once: the loader of nfc_kernels.hip, nfc_envelope.hip
 * and nfc_wave.hip (which each had a copy of it), the conversions their row fetches apply, and the byte arithmetic of the host
 * runtime (nfcgpu.hip). It compiles for the device and for the host (tests/test_sample_loader.py checks it with g++ against
 * numpy, value by value), as nfc_spectrum.hpp does.
 *
 * Sample layout. A submission has one layout, carried in the fields that carried the floats per sample so far
 * (NfcLaunch::uniformStride, NfcScanArgs::stride, NfcWork::stride, the wave decoder's deep.stride):
 *
 *     bits 0-7   components per sample: 1 magnitude, 2 interleaved I/Q
 *     bit  8     NFC_SAMPLE_I16: the components are little-endian int16 PCM instead of float
 *
 * so float input keeps the values those fields have always held (1, 2) and whoever knows floats only - the emulated twins under
 * tests/hostsim - goes on reading them as they are; int16 input is 0x101 (mono) and 0x102 (I/Q). A layout is uniform over a
 * launch: every choice made on it is a scalar branch or a template parameter, never a per-lane one. The kernels that read samples
 * exist once per format (nfc_demod_kernel / nfc_demod_kernel_i16, ...; the host picks by the layout), so inside a kernel only
 * magnitude against IQ is left to decide.
 *
 * int16 -> float is (float)v / 32768.0f (hw::RecordDevice::readScaledSamples<short>, RecordDevice.cpp:247-248, 297-300), written
 * here as the product with 2^-15: both are exact for every int16, so they are the same float. I/Q components are converted
 * first and then go through nfc_iq_magnitude like float ones.
 */
#ifndef NFC_SAMPLE_HPP
#define NFC_SAMPLE_HPP

#include <stdint.h>

#ifdef __HIPCC__
#define NFC_SAMPLE_FN __host__ __device__ __forceinline__
#else
#define NFC_SAMPLE_FN static inline
#endif

#define NFC_SAMPLE_I16 0x100u

/* components per sample of a layout: 1 magnitude, 2 I/Q */
NFC_SAMPLE_FN uint32_t nfc_sample_components(uint32_t layout)
{
   return layout & 0xFFu;
}

/* bytes per sample of a layout: 4 / 8 (float), 2 / 4 (int16) */
NFC_SAMPLE_FN uint32_t nfc_sample_bytes(uint32_t layout)
{
   return nfc_sample_components(layout) * ((layout & NFC_SAMPLE_I16) ? 2u : 4u);
}

NFC_SAMPLE_FN float nfc_i16_to_float(int16_t v)
{
   return (float)v * (1.0f / 32768.0f);
}

/* an I/Q sample as it lies in memory: rows are aligned to a sample, so one 64-bit (float) or one 32-bit (int16) load */
struct alignas(8) NfcIq32
{
   float i, q;
};

struct alignas(4) NfcIq16
{
   int16_t i, q;
};

/* magnitude of one IQ sample, the reference's scalar formula (RadioDeviceTask.cpp:626-642): products and sum rounded
 * separately (no contraction), correctly rounded square root */
NFC_SAMPLE_FN float nfc_iq_magnitude(float i, float q)
{
#if defined(__HIP_DEVICE_COMPILE__)
   return __builtin_sqrtf(__fadd_rn(__fmul_rn(i, i), __fmul_rn(q, q)));
#else
   /* (host: built with -ffp-contract=off, the plain operators are the rounded ones) */
   const float ii = i * i, qq = q * q;
   return __builtin_sqrtf(ii + qq);
#endif
}

/* Sample `index` of a row that starts at `data`, as a magnitude, for a caller that is compiled for one format (I16: int16 PCM,
 * else float) and only has to tell magnitude from IQ - the kernels, which exist once per format so that the float ones are the
 * code they were before there was a second format. `layout` is uniform. */
template <bool I16>
NFC_SAMPLE_FN float nfc_sample_at_as(const uint8_t *data, uint32_t layout, uint32_t index)
{
   if (I16)
   {
      if (layout == (NFC_SAMPLE_I16 | 2u))
      {
         const NfcIq16 iq = reinterpret_cast<const NfcIq16 *>(data)[index];
         return nfc_iq_magnitude(nfc_i16_to_float(iq.i), nfc_i16_to_float(iq.q));
      }

      /* (a mono row may start at any sample: a 16-bit load) */
      return nfc_i16_to_float(reinterpret_cast<const int16_t *>(data)[index]);
   }

   if (layout == 2u)
   {
      const NfcIq32 iq = reinterpret_cast<const NfcIq32 *>(data)[index];
      return nfc_iq_magnitude(iq.i, iq.q);
   }

   return reinterpret_cast<const float *>(data)[index];
}

/* the same for any layout */
NFC_SAMPLE_FN float nfc_sample_at(const uint8_t *data, uint32_t layout, uint32_t index)
{
   return (layout & NFC_SAMPLE_I16) ? nfc_sample_at_as<true>(data, layout, index) : nfc_sample_at_as<false>(data, layout, index);
}

#endif
