/*
 * nfc_tap_reduce.hpp - nfcgpu_signal_tap_reduce, held once: the planes of the tap (nfc_tap.hpp) reduced over sample ranges to
 * min, max, where they lie, the mean and the count of values that are no NaN. The device kernels (nfc_tap_reduce.hip) and
 * their CPU twins of the emulated test build (nfcgpu.hip, NFCGPU_EMULATED_TEST_BUILD) compile this text, as with nfc_record.hpp.
 *
 * Shape. The host runs the tap over a slab of whole buffers b0 ... b1 - 1 into planes of its own and then reduces the ranges
 * that lie in those buffers (an item: a range of the pass). A range is cut into segments of kSegment samples by offset within
 * the range; a wave takes one unit - (item, segment, channel) - and leaves one partial; a thread of the finishing kernel merges
 * a range's partials in segment order into the record. Within a segment lane l takes the quads l, l + 64, ... (a quad: four
 * consecutive offsets). Everything is laid out by a sample's offset within its range, never by where the range lies in the
 * buffer or in memory, so a record does not depend on the other ranges, on the slabs or on alignment.
 *
 * Which units a pass has is the host's plan, never the caller's data: with bins every range has segsPerBin segments; with
 * explicit ranges `order` lists the ranges by buffer, prefix[o] is the number of segments ahead of order[o] and `table` names every
 * segment in that order, so a wave finds its unit with one load. The range itself is
 * read where the caller left it and checked here (nfc_tap_range_ok) before a sample is read: a range that is not inside the
 * buffers of the pass reads nothing, gets the empty record and raises the flag.
 *
 * mean: values widen to double (exact); a quad is (v0 + v1) + (v2 + v3) with 0 for a NaN or a missing sample (adding 0 is exact),
 * the lane adds its quads in sequence (at most kIters = 64, the first to 0: 63 roundings), a butterfly over the wave (6), the
 * segments in sequence (segments - 1). A value of a range of N samples meets at most 2 + (ceil(N / 256) - 1) + 6 roundings in
 * one segment, 71 + (segments - 1) in several: never more than ceil(N / 64) + 7.
 */
#ifndef NFC_TAP_REDUCE_HPP
#define NFC_TAP_REDUCE_HPP

#include <stdint.h>

#include "nfc_sample.hpp"

#define NFC_TAP_REDUCE_FN NFC_SAMPLE_FN

#define NFC_TAP_NONE 0xFFFFFFFFu       /* argmin / argmax of nothing */
#define NFC_TAP_NAN_BITS 0x7FC00000u   /* min, max and mean of nothing */

struct NfcTapReduceShape
{
   static constexpr uint32_t kSegment = 16384;             /* samples */
   static constexpr uint32_t kSegmentQuads = kSegment / 4;
   static constexpr uint32_t kIters = kSegmentQuads / 64;  /* quads of a lane */
   static constexpr uint32_t kWaves = 4;                   /* of a workgroup; each on a unit of its own */
};

/* nfcgpu_tap_range */
struct NfcTapRange
{
   uint32_t buffer, first, count, reserved;
};

/* nfcgpu_tap_stat */
struct NfcTapStat
{
   float min, max, mean;
   uint32_t valid;
   uint32_t argmin, argmax;
   uint32_t reserved[2];
};

/* what a lane, a wave, a segment knows; minI / maxI == NFC_TAP_NONE: nothing seen yet */
struct NfcTapPartial
{
   double sum;
   float minV, maxV;
   uint32_t minI, maxI;
   uint32_t valid, pad;
};

/* a segment of the plan */
struct NfcTapSegment
{
   uint32_t range, segment;
};

struct NfcTapReduceArgs
{
   const float *planes;          /* of the buffers b0 ... b1 - 1: buffer b, channel k at (b - b0) * bufferPitch + k * planePitch */
   const NfcTapRange *ranges;    /* the caller's, or null: bins */
   const uint32_t *order;        /* ranges mode: range indices by buffer; item i of the pass is order[firstItem + i] */
   const uint64_t *prefix;       /* ranges mode: [nRanges + 1], segments ahead of order[o] */
   const NfcTapSegment *table;   /* ranges mode: [prefix[nRanges]], the segments in that order */
   NfcTapPartial *partials;      /* [units] */
   NfcTapStat *out;              /* [records]: range r, channel k at r * channels + k */
   uint32_t *flag;               /* set when a range is refused */
   uint64_t bufferPitch, planePitch; /* bytes */
   uint64_t units;               /* of the pass: segments * channels */
   uint64_t items, firstItem;    /* ranges of the pass; bins mode: firstItem = b0 * bins */
   uint64_t prefix0;             /* ranges mode: prefix[firstItem] */
   uint32_t n, nBuffers;
   uint32_t b0, b1;
   uint32_t channels;            /* how many are selected */
   uint32_t binSamples, bins, segsPerBin;
};

/* four floats wherever a float may lie */
struct __attribute__((packed, aligned(4))) NfcTapFloat4
{
   float v[4];
};

NFC_TAP_REDUCE_FN float nfc_tap_nan()
{
   union { uint32_t u; float f; } b;
   b.u = NFC_TAP_NAN_BITS;
   return b.f;
}

NFC_TAP_REDUCE_FN uint32_t nfc_tap_segments(uint32_t count)
{
   return (uint32_t)(((uint64_t)count + NfcTapReduceShape::kSegment - 1) / NfcTapReduceShape::kSegment);
}

NFC_TAP_REDUCE_FN void nfc_tap_partial_begin(NfcTapPartial &p)
{
   p.sum = 0.0;
   p.minV = nfc_tap_nan();
   p.maxV = nfc_tap_nan();
   p.minI = NFC_TAP_NONE;
   p.maxI = NFC_TAP_NONE;
   p.valid = 0;
   p.pad = 0;
}

/* a and b of disjoint sets of samples: the smaller value, of equal ones (-0.0 and 0.0 are) the one at the lower index */
NFC_TAP_REDUCE_FN NfcTapPartial nfc_tap_partial_merge(const NfcTapPartial &a, const NfcTapPartial &b)
{
   NfcTapPartial r = a;

   if (b.minI != NFC_TAP_NONE && (a.minI == NFC_TAP_NONE || b.minV < a.minV || (b.minV == a.minV && b.minI < a.minI)))
   {
      r.minV = b.minV;
      r.minI = b.minI;
   }
   if (b.maxI != NFC_TAP_NONE && (a.maxI == NFC_TAP_NONE || b.maxV > a.maxV || (b.maxV == a.maxV && b.maxI < a.maxI)))
   {
      r.maxV = b.maxV;
      r.maxI = b.maxI;
   }

   r.sum = a.sum + b.sum;
   r.valid = a.valid + b.valid;
   return r;
}

/* sample `index` (higher than any the lane has seen) with value v; its share of the sum: 0 for a NaN */
NFC_TAP_REDUCE_FN double nfc_tap_partial_take(NfcTapPartial &p, float v, uint32_t index)
{
   if (v != v)
      return 0.0;

   if (p.minI == NFC_TAP_NONE || v < p.minV)
   {
      p.minV = v;
      p.minI = index;
   }
   if (p.maxI == NFC_TAP_NONE || v > p.maxV)
   {
      p.maxV = v;
      p.maxI = index;
   }

   p.valid++;
   return (double)v;
}

/* the record of a range whose partials are all in p */
NFC_TAP_REDUCE_FN NfcTapStat nfc_tap_stat(const NfcTapPartial &p)
{
   NfcTapStat s;

   s.min = p.minV;
   s.max = p.maxV;
   s.mean = p.valid ? (float)(p.sum / (double)p.valid) : nfc_tap_nan();
   s.valid = p.valid;
   s.argmin = p.minI;
   s.argmax = p.maxI;
   s.reserved[0] = 0;
   s.reserved[1] = 0;
   return s;
}

/* the range whose records have the index r */
NFC_TAP_REDUCE_FN NfcTapRange nfc_tap_reduce_range(const NfcTapReduceArgs &A, uint32_t r)
{
   NfcTapRange g;

   if (A.ranges)
      return A.ranges[r];

   g.buffer = r / A.bins;
   g.first = (r % A.bins) * A.binSamples;
   g.count = A.n - g.first < A.binSamples ? A.n - g.first : A.binSamples;
   g.reserved = 0;
   return g;
}

/* inside the buffers of the call? */
NFC_TAP_REDUCE_FN bool nfc_tap_range_ok(const NfcTapReduceArgs &A, const NfcTapRange &g)
{
   return g.buffer < A.nBuffers && g.reserved == 0 && g.first <= A.n && g.count <= A.n - g.first;
}

/* unit j of the pass: channel fastest, then the segments of the pass in item order */
NFC_TAP_REDUCE_FN void nfc_tap_reduce_unit(const NfcTapReduceArgs &A, uint64_t j, uint32_t &r, uint32_t &segment, uint32_t &k)
{
   const uint64_t t = j / A.channels;

   k = (uint32_t)(j % A.channels);

   if (A.ranges)
   {
      const NfcTapSegment u = A.table[A.prefix0 + t];

      r = u.range;
      segment = u.segment;
   }
   else
   {
      r = (uint32_t)(A.firstItem + t / A.segsPerBin);
      segment = (uint32_t)(t % A.segsPerBin);
   }
}

/* Lane `lane` of the wave that has unit j: its quads of the segment. Nothing is read of a range that is not inside the planes
 * of the pass, nor beyond a range's count. */
NFC_TAP_REDUCE_FN NfcTapPartial nfc_tap_reduce_lane(const NfcTapReduceArgs &A, uint64_t j, uint32_t lane)
{
   NfcTapPartial acc;
   nfc_tap_partial_begin(acc);

   uint32_t r, segment, k;

   nfc_tap_reduce_unit(A, j, r, segment, k);

   const NfcTapRange g = nfc_tap_reduce_range(A, r);

   if (!nfc_tap_range_ok(A, g) || g.buffer < A.b0 || g.buffer >= A.b1 || segment >= nfc_tap_segments(g.count))
      return acc;

   const uint32_t begin = segment * NfcTapReduceShape::kSegment;      /* offset within the range; < count <= 2^32 - 1 */
   const uint32_t left = g.count - begin;
   const uint32_t len = left < NfcTapReduceShape::kSegment ? left : NfcTapReduceShape::kSegment;
   const uint32_t quads = (len + 3) / 4;
   const uint32_t at = g.first + begin;                               /* sample of the buffer */
   const float *plane = reinterpret_cast<const float *>(reinterpret_cast<const uint8_t *>(A.planes) + (uint64_t)(g.buffer - A.b0) * A.bufferPitch +
                                                        (uint64_t)k * A.planePitch) + at;

   for (uint32_t q = lane; q < quads; q += 64)
   {
      const uint32_t o = q * 4;
      double d[4] = {0.0, 0.0, 0.0, 0.0};

      if (len - o >= 4)
      {
         /* (a range starts at any sample: a 16-byte load of a dword-aligned address) */
         const NfcTapFloat4 v = *reinterpret_cast<const NfcTapFloat4 *>(plane + o);

         for (uint32_t p = 0; p < 4; p++)
            d[p] = nfc_tap_partial_take(acc, v.v[p], at + o + p);
      }
      else
      {
         for (uint32_t p = 0; p < len - o; p++)
            d[p] = nfc_tap_partial_take(acc, plane[o + p], at + o + p);
      }

      acc.sum = acc.sum + ((d[0] + d[1]) + (d[2] + d[3]));
   }

   return acc;
}

/* record t of the pass - (item, channel), channel fastest - from the range's partials in segment order */
NFC_TAP_REDUCE_FN void nfc_tap_reduce_finish(const NfcTapReduceArgs &A, uint64_t t)
{
   const uint64_t item = t / A.channels;
   const uint32_t k = (uint32_t)(t % A.channels);
   const uint32_t r = A.ranges ? A.order[A.firstItem + item] : (uint32_t)(A.firstItem + item);
   const NfcTapRange g = nfc_tap_reduce_range(A, r);
   const bool ok = nfc_tap_range_ok(A, g);

   NfcTapPartial acc;
   nfc_tap_partial_begin(acc);

   if (ok)
   {
      /* (the segments the plan gave the range: what nfc_tap_segments(count) says while nobody rewrites the ranges under the call) */
      const uint64_t base = A.ranges ? A.prefix[A.firstItem + item] - A.prefix0 : item * A.segsPerBin;
      const uint64_t segments = A.ranges ? A.prefix[A.firstItem + item + 1] - A.prefix[A.firstItem + item] : nfc_tap_segments(g.count);

      for (uint64_t s = 0; s < segments; s++)
         acc = nfc_tap_partial_merge(acc, A.partials[(base + s) * A.channels + k]);
   }
   else
      *A.flag = 1u;

   A.out[(uint64_t)r * A.channels + k] = nfc_tap_stat(acc);
}

#endif
