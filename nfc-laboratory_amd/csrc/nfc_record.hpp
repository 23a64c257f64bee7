/*
 * nfc_record.hpp - arithmetic of nfcgpu_record, held once: float samples to the int16 PCM of a capture file
 * (hw::RecordDevice::writeScaledSamples<short>, RecordDevice.cpp:313-348) and the levels of the receiver
 * (RadioDeviceTask::processQueue, RadioDeviceTask.cpp:547-680). The device kernels (nfc_record.hip) and their CPU twins of the
 * emulated test build (nfcgpu.hip, NFCGPU_EMULATED_TEST_BUILD) compile this text, as with nfc_spectrum.hpp.
 *
 * Shape. A buffer is cut into segments of kSegmentSamples samples; a workgroup of kWaves waves takes one segment, a wave a run
 * of kIters * 64 quads (a quad: four consecutive samples, 4 q ... 4 q + 3 of the buffer), lane l of the wave the quads
 * l, l + 64, ... of that run. Everything about levels is laid out by sample index, never by where a row lies in memory, so a
 * buffer's levels do not depend on its alignment or on its neighbours.
 *
 * power: squares (I * I + Q * Q: one addition), the quad (s0 + s1) + (s2 + s3) (two), the lane's kIters quads in sequence
 * (16), a butterfly over the wave (6), the waves (p0 + p1) + (p2 + p3) (2), then the segments of a buffer in groups of 64, groups
 * of groups, ... (at most 18 for 2^32 samples): 45 additions at most on any value's way.
 *
 * average: a = 0; a = a * w0 + m[4 k] * w1 over the K = ceil(n / 4) quads of a buffer is sum_k m[4 k] w1 w0^(K - 1 - k). A lane
 * runs the recurrence over its own quads with w0^64 for w0 (they are 64 quads apart), its result is weighted with
 * w0^(63 - lane) and the wave's with w0^(64 kIters (kWaves - 1 - wave)), so a segment's sum stands as if the segment were
 * full: the last, short one is put right with w0^-(missing quads), and the segments are chained in index order,
 * a = a_left * w0^(K_right) + a_right. Every power of w0 comes from the host, computed in double (NfcRecordWeights).
 * Each term meets about 60 roundings at the very most, well inside the 2048 the contract allows.
 */
#ifndef NFC_RECORD_HPP
#define NFC_RECORD_HPP

#include <stdint.h>

#include "nfc_sample.hpp"

#define NFC_RECORD_FN NFC_SAMPLE_FN

#define NFC_RECORD_SAME 0
#define NFC_RECORD_MAGNITUDE 1

struct NfcRecordShape
{
   static constexpr uint32_t kWaves = 4;
   static constexpr uint32_t kIters = 16;
   static constexpr uint32_t kThreads = 64 * kWaves;
   static constexpr uint32_t kWaveQuads = 64 * kIters;
   static constexpr uint32_t kSegmentQuads = kWaveQuads * kWaves;
   static constexpr uint32_t kSegmentSamples = 4 * kSegmentQuads; /* 16 384 */
};

/* what a lane, a wave, a segment knows of the levels */
struct NfcRecordPartial
{
   float power;      /* sum of squares */
   float average;    /* weighted towards the end of the (full) segment */
   float peak;       /* NaN: nothing seen yet */
   uint32_t clipped;
};

struct NfcRecordWeights
{
   float w1;         /* 0.001f */
   float w64;        /* w0^64, w0 = 1 - 0.001f */
   float segment;    /* w0^kSegmentQuads */
   float last;       /* w0^(quads of the last segment) */
   float unpad;      /* w0^-(kSegmentQuads - quads of the last segment) */
   float wave[NfcRecordShape::kWaves]; /* w0^(kWaveQuads * (kWaves - 1 - wave)) */
   float lane[64];   /* w0^(63 - lane) */
};

struct NfcRecordArgs
{
   const float *in;
   int16_t *out;
   NfcRecordPartial *partials;  /* [nBuffers * nSegments], levels only */
   NfcRecordPartial *levels;    /* [nBuffers]: nfcgpu_record_levels has this layout */
   uint64_t inPitch, outPitch;  /* bytes */
   uint64_t total;              /* nBuffers * nSegments */
   uint32_t nSegments;          /* per buffer */
   uint32_t n;                  /* samples per buffer */
   uint32_t nBuffers;
   NfcRecordWeights w;
};

/* four floats wherever a float may lie */
struct __attribute__((packed, aligned(4))) NfcRecordFloat4
{
   float v[4];
};

NFC_RECORD_FN float nfc_record_nan()
{
   return __builtin_nanf("");
}

/* the largest of what is not NaN (fmaxf: a NaN operand yields the other one) */
NFC_RECORD_FN float nfc_record_max(float a, float b)
{
   return __builtin_fmaxf(a, b);
}

/* one value to PCM: t = v * 32768 (exact but for overflow), toward zero; beyond the range the ends, NaN 0, both counted */
NFC_RECORD_FN int32_t nfc_record_quantise(float v, uint32_t &clipped)
{
   const float t = v * 32768.0f;

   if (t != t)
   {
      clipped++;
      return 0;
   }
   if (t >= 32768.0f)
   {
      clipped++;
      return 32767;
   }
   if (t <= -32769.0f)
   {
      clipped++;
      return -32768;
   }
   return (int32_t)t;
}

NFC_RECORD_FN void nfc_record_begin(NfcRecordPartial &p)
{
   p.power = 0;
   p.average = 0;
   p.peak = nfc_record_nan();
   p.clipped = 0;
}

/* channels of the PCM a (stride, mode) writes */
template <int STRIDE, int MODE>
struct NfcRecordKind
{
   static constexpr int kChannels = (STRIDE == 2 && MODE == NFC_RECORD_SAME) ? 2 : 1;
};

/* One quad: `valid` (1 ... 4) samples at `src`. e[p] is what sample p is written as - the int16 of a mono sample, or the pair of
 * an I/Q sample packed as it lies in memory (I low) - and with LEVELS the lane's partial takes the quad in. A sample that is
 * not there is written as 0 and takes no part in the levels. */
template <int STRIDE, int MODE, bool LEVELS>
NFC_RECORD_FN void nfc_record_quad(const float *src, uint32_t valid, uint32_t e[4], NfcRecordPartial &acc, const NfcRecordWeights &w)
{
   float v[4 * STRIDE];

   if (valid == 4)
   {
      for (int j = 0; j < STRIDE; j++)
      {
         const NfcRecordFloat4 f = reinterpret_cast<const NfcRecordFloat4 *>(src)[j];
         for (int c = 0; c < 4; c++)
            v[4 * j + c] = f.v[c];
      }
   }
   else
   {
      for (uint32_t c = 0; c < 4 * STRIDE; c++)
         v[c] = c < valid * STRIDE ? src[c] : 0.0f;
   }

   float square[4], m0 = 0;
   uint32_t clipped = 0;

   for (uint32_t p = 0; p < 4; p++)
   {
      float m = 0;

      if (STRIDE == 2)
      {
         const float i = v[2 * p], q = v[2 * p + 1];

         if (LEVELS || MODE == NFC_RECORD_MAGNITUDE)
            m = nfc_iq_magnitude(i, q);
         if (LEVELS)
         {
            const float ii = i * i, qq = q * q;
            square[p] = ii + qq;
         }

         if (MODE == NFC_RECORD_MAGNITUDE)
            e[p] = (uint32_t)nfc_record_quantise(m, clipped) & 0xFFFFu;
         else
         {
            const uint32_t lo = (uint32_t)nfc_record_quantise(i, clipped) & 0xFFFFu;
            e[p] = lo | ((uint32_t)nfc_record_quantise(q, clipped) << 16);
         }
      }
      else
      {
         m = v[p];
         if (LEVELS)
            square[p] = m * m;
         e[p] = (uint32_t)nfc_record_quantise(m, clipped) & 0xFFFFu;
      }

      if (LEVELS && p < valid)
         acc.peak = nfc_record_max(acc.peak, m);
      if (p == 0)
         m0 = m;
   }

   if (LEVELS)
   {
      /* (samples that are not there were read as 0: their squares add nothing and they clip nothing) */
      acc.power = acc.power + ((square[0] + square[1]) + (square[2] + square[3]));
      acc.average = acc.average * w.w64 + m0 * w.w1;
      acc.clipped += clipped;
   }
}

/* a lane with no quad at that step: the recurrence still moves on */
NFC_RECORD_FN void nfc_record_quad_none(NfcRecordPartial &acc, const NfcRecordWeights &w)
{
   acc.average = acc.average * w.w64;
}

/* a lane's partial as it enters the wave's sum */
NFC_RECORD_FN void nfc_record_lane_end(NfcRecordPartial &acc, uint32_t lane, const NfcRecordWeights &w)
{
   acc.average = acc.average * w.lane[lane];
}

NFC_RECORD_FN NfcRecordPartial nfc_record_add(const NfcRecordPartial &a, const NfcRecordPartial &b)
{
   NfcRecordPartial r;
   r.power = a.power + b.power;
   r.average = a.average + b.average;
   r.peak = nfc_record_max(a.peak, b.peak);
   r.clipped = a.clipped + b.clipped;
   return r;
}

/* the waves of a workgroup, in wave order */
NFC_RECORD_FN NfcRecordPartial nfc_record_segment(const NfcRecordPartial *waves, const NfcRecordWeights &w)
{
   NfcRecordPartial p[NfcRecordShape::kWaves];

   for (uint32_t i = 0; i < NfcRecordShape::kWaves; i++)
   {
      p[i] = waves[i];
      p[i].average = p[i].average * w.wave[i];
   }

   return nfc_record_add(nfc_record_add(p[0], p[1]), nfc_record_add(p[2], p[3]));
}

/* the chain of a buffer's segment averages, in index order */
NFC_RECORD_FN float nfc_record_chain_average(const NfcRecordPartial *segments, uint32_t nSegments, const NfcRecordWeights &w)
{
   float a = 0;

   for (uint32_t s = 0; s < nSegments; s++)
   {
      if (s + 1 < nSegments)
         a = a * w.segment + segments[s].average;
      else
         a = a * w.last + segments[s].average * w.unpad;
   }

   return a;
}

/* what a buffer's record holds, of the sums over its segments */
NFC_RECORD_FN NfcRecordPartial nfc_record_levels(float power, float average, float peak, uint32_t clipped, uint32_t n)
{
   NfcRecordPartial r;
   r.power = power / (float)n;
   r.average = average;
   r.peak = peak != peak ? 0.0f : peak + 0.0f; /* (-0 and +0 compare equal: one of them) */
   r.clipped = clipped;
   return r;
}

#endif
