/*
 * nfc_resample.hpp - the adaptive resampler (SignalResamplingTask.cpp:168-226, `processRadioSignal`) for the sample layouts the
 * float-magnitude kernel of nfc_kernels.hip does not read: int16 magnitude, int16 I/Q and float I/Q (nfc_sample.hpp). Held once: the
 * device kernels (nfc_resample.hip) and their CPU twins of the emulated test build (nfcgpu.hip, NFCGPU_EMULATED_TEST_BUILD) compile
 * this text.
 *
 * The work of a buffer is what it is in nfc_resample_radio_kernel, and so is its shape: the running mean is a sequential fp32 sum
 * (add the sample entering the centred window, subtract the one leaving it, in that order), so a buffer is one lane's work and 64
 * buffers share a wave. Rows are staged kTile samples at a time into a per-lane ring of floats in LDS that always holds the
 * 51-sample window of the sample being decided; a sample is decided once the 25 samples behind it are there. The one thing that
 * differs is the staging: a sample becomes a float - the magnitude the decoder's loader forms of the same bytes (nfc_sample.hpp:
 * nfc_i16_to_float, nfc_iq_magnitude) - on its way into the ring, and the next tile is fetched while this one is decided. From the
 * ring on the decision loop reads floats and takes the operations of the float kernel in the order of the float kernel, so the
 * control points are bit for bit those nfcgpu_resample_radio gives for those magnitudes.
 *
 * Ring and tile keep the float kernel's invariants (NfcResampleShape): the ring is a multiple of the tile and at least window + tile,
 * so the tile being staged never lies on a sample the decisions still read (the oldest one read while the tile at `base` is staged
 * is base - 51, the youngest overwritten base - 65). The ring's pitch is odd: lanes read their own rows without bank conflicts, and
 * the staging stores of a half wave are 32 consecutive floats of one row.
 */
#ifndef NFC_RESAMPLE_HPP
#define NFC_RESAMPLE_HPP

#include <stdint.h>

#include "nfc_sample.hpp"

struct NfcResampleShape
{
   static constexpr int kWindow = 51;     /* WINDOW */
   static constexpr int kInterval = 255;  /* RADIO_INTERVAL */
   static constexpr uint32_t kLanes = 64; /* buffers per workgroup, one wave */
   static constexpr uint32_t kTile = 32;  /* samples staged per pass */
   static constexpr uint32_t kRing = 96;  /* per-lane sample window in LDS */
   static constexpr uint32_t kPitch = 97;

   static_assert(kRing % kTile == 0 && kRing >= kWindow + kTile, "the ring: a multiple of the tile, at least window + tile");
   static_assert(kPitch > kRing && (kPitch & 1), "the pitch: odd, beyond the ring");
};

struct NfcResampleArgs
{
   const uint8_t *in;  /* buffer b starts at in + b * inPitchBytes, n samples of `layout` */
   float *out;         /* control points of buffer b: pairs at out + b * outPitchFloats (8-byte aligned rows) */
   uint32_t *counts;
   uint64_t inPitchBytes;
   uint64_t outPitchFloats;
   uint32_t nBuffers;
   uint32_t n;
   uint32_t capacityPairs;
   uint32_t layout;    /* nfc_sample.hpp; uniform, and the kernels are compiled per layout */
};

struct alignas(8) NfcResamplePair
{
   float value, offset;
};

/* what a buffer's lane carries from sample to sample */
struct NfcResampleLane
{
   float avrg, last;
   int32_t i, c, p;
   uint32_t posI, posA, posR; /* ring columns of i, of the sample entering the window and of the one leaving it */
   uint32_t count;
};

NFC_SAMPLE_FN void nfc_resample_begin(NfcResampleLane &s)
{
   s.avrg = 0.0f;
   s.last = 0.0f;
   s.i = 0;
   s.c = 0;
   s.p = -1;
   s.posI = 0;
   s.posA = NfcResampleShape::kWindow / 2;
   s.posR = NfcResampleShape::kRing - (NfcResampleShape::kWindow / 2) - 1;
   s.count = 0;
}

NFC_SAMPLE_FN void nfc_resample_put(const NfcResampleArgs &A, uint32_t buffer, bool mine, NfcResampleLane &s, float value, float offset)
{
   if (mine && s.count < A.capacityPairs)
   {
      NfcResamplePair pair;
      pair.value = value;
      pair.offset = offset;
      reinterpret_cast<NfcResamplePair *>(A.out + (uint64_t)buffer * A.outPitchFloats)[s.count] = pair;
   }

   s.count++;
}

/* A sample as it lies in a row, per layout, and the float the ring holds of it: the conversion and the magnitude of the decoder's
 * loader (nfc_sample_at_as: nfc_i16_to_float, nfc_iq_magnitude). Fetching and converting are two steps so that a kernel can have
 * the loads of a whole tile in flight before it converts the first value. */
template <uint32_t LAYOUT> struct NfcResampleRaw;
template <> struct NfcResampleRaw<NFC_SAMPLE_I16 | 1u> { typedef int16_t Type; };
template <> struct NfcResampleRaw<NFC_SAMPLE_I16 | 2u> { typedef NfcIq16 Type; };
template <> struct NfcResampleRaw<2u> { typedef NfcIq32 Type; };

NFC_SAMPLE_FN float nfc_resample_value(int16_t raw) { return nfc_i16_to_float(raw); }
NFC_SAMPLE_FN float nfc_resample_value(NfcIq16 raw) { return nfc_iq_magnitude(nfc_i16_to_float(raw.i), nfc_i16_to_float(raw.q)); }
NFC_SAMPLE_FN float nfc_resample_value(NfcIq32 raw) { return nfc_iq_magnitude(raw.i, raw.q); }

/* (beyond the buffer, and for a lane without one, sample 0 of buffer 0 is read instead - it is always there - and dropped by
 * nfc_resample_settle: a load without a branch around it, so that nothing keeps the loads of a tile from being issued together) */
template <uint32_t LAYOUT>
NFC_SAMPLE_FN typename NfcResampleRaw<LAYOUT>::Type nfc_resample_fetch(const NfcResampleArgs &A, uint32_t buffer, uint32_t idx)
{
   const bool there = buffer < A.nBuffers && idx < A.n;
   const uint64_t row = there ? buffer : 0u;
   const uint32_t at = there ? idx : 0u;

   return reinterpret_cast<const typename NfcResampleRaw<LAYOUT>::Type *>(A.in + row * A.inPitchBytes)[at];
}

/* what the ring holds of sample idx of a buffer: the magnitude; 0 beyond the buffer and for a lane without one */
template <uint32_t LAYOUT>
NFC_SAMPLE_FN float nfc_resample_settle(const NfcResampleArgs &A, uint32_t buffer, uint32_t idx, typename NfcResampleRaw<LAYOUT>::Type raw)
{
   return buffer < A.nBuffers && idx < A.n ? nfc_resample_value(raw) : 0.0f;
}

template <uint32_t LAYOUT>
NFC_SAMPLE_FN float nfc_resample_sample(const NfcResampleArgs &A, uint32_t buffer, uint32_t idx)
{
   return nfc_resample_settle<LAYOUT>(A, buffer, idx, nfc_resample_fetch<LAYOUT>(A, buffer, idx));
}

/* after the tile at `base` has been staged: decide every sample whose window is complete (all of them once the buffer has been
 * read to its end). `window` is the lane's row of the ring. */
NFC_SAMPLE_FN void nfc_resample_decide(const NfcResampleArgs &A, uint32_t buffer, bool mine, NfcResampleLane &s, const float *window, uint32_t base)
{
   constexpr int32_t W = NfcResampleShape::kWindow;
   const float filter = 0.005f; /* THRESHOLD */
   const uint32_t n = A.n;
   const uint32_t filled = base + NfcResampleShape::kTile < n ? base + NfcResampleShape::kTile : n;

   if (base == 0)
   {
      /* "initialize average" and "always store first sample" */
      for (uint32_t k = 0; k < (uint32_t)(W / 2); k++)
         s.avrg += window[k];

      s.last = window[0];
      nfc_resample_put(A, buffer, mine, s, window[0], 0.0f);
   }

   const int32_t stop = filled == n ? (int32_t)n : (int32_t)filled - W / 2;

   for (; s.i < stop; ++s.i, ++s.p)
   {
      const float value = window[s.posI];

      if ((uint32_t)(s.i + W / 2) < n)
         s.avrg += window[s.posA];

      if (s.i - W / 2 - 1 >= 0)
         s.avrg -= window[s.posR];

      const float stdev = __builtin_fabsf(value - (s.avrg / (float)W));

      if (stdev > filter || (s.i - s.c) >= NfcResampleShape::kInterval)
      {
         if (stdev > filter && s.c < s.p)
            nfc_resample_put(A, buffer, mine, s, s.last, (float)s.p);

         nfc_resample_put(A, buffer, mine, s, value, (float)s.i);

         s.c = s.i;
      }

      s.last = value;

      s.posI = s.posI + 1 == NfcResampleShape::kRing ? 0 : s.posI + 1;
      s.posA = s.posA + 1 == NfcResampleShape::kRing ? 0 : s.posA + 1;
      s.posR = s.posR + 1 == NfcResampleShape::kRing ? 0 : s.posR + 1;
   }
}

/* behind the last tile: the sample before the end, the count */
NFC_SAMPLE_FN void nfc_resample_end(const NfcResampleArgs &A, uint32_t buffer, bool mine, NfcResampleLane &s)
{
   if (s.c < s.p)
      nfc_resample_put(A, buffer, mine, s, s.last, (float)s.p);

   if (mine)
      A.counts[buffer] = s.count;
}

#endif
