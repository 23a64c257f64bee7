/*
 * nfc_apcm.hpp - nfcgpu_apcm_encode, held once: the resampler's control points (nfc_resample.hpp) delta-coded into the
 * "radio-<id>.apcm" entries of a trace file, as the reference's TraceStorageTask::writeRadioEntry stores them
 * (lab-tasks/src/main/cpp/tasks/TraceStorageTask.cpp:881-1003, read back by readRadioEntry :760-879). The device kernels
 * (nfc_apcm.hip) and their CPU twins of the emulated test build (nfcgpu.hip, NFCGPU_EMULATED_TEST_BUILD) compile this text, as with
 * nfc_tap_reduce.hpp.
 *
 * Semantics. G consecutive buffers are one entry; buffer j of an entry has the stream position p_j = firstPosition + j *
 * bufferSamples (hw::SignalBuffer::offset()). sampleStart = (uint32)(sampleRate * rangeStart), sampleEnd = (uint32)(sampleRate *
 * rangeEnd), the reference's double product and cast (:907-908); rangeStart == rangeEnd == 0 means every point (sampleStart 0,
 * sampleEnd 2^32 - 1), the departure nfcgpu_trace_write_frames makes for frames. Point by point, in buffer order and then in pair
 * order (:957-970):
 *    offset = p_j + (uint32)pair.offset   (a negative value or a NaN gives 0, the cast saturates above; the sum is taken mod 2^32)
 *    sample = nfc_record_quantise(pair.value): static_cast<short>(v * 32768.0f) in range (:969), saturated beyond it, NaN as 0 -
 *             the quantiser and the departure of nfcgpu_record (nfc_record.hpp).
 * A point is kept iff sampleStart <= offset <= sampleEnd. For the monotone offsets the resampler produces this is the reference's
 * `continue` below the range and `break` above it (:972-976): nothing behind the first point above sampleEnd is inside the range.
 * Kept point k becomes three bytes (:979-981): (offset_k - offset_{k-1}) & 0xff, then (sample_k - sample_{k-1}) & 0xffff, low byte
 * first, with offset_{-1} = sampleStart and sample_{-1} = 0 (:953-954). The entry is the 32-byte SampleHdr (:55-60, indices
 * :36-39) - "APCM", version 2, info = {0, 0 (start offset: the reference writes 0, :912), K, stream id, sampleRate, 0} - and the K
 * records behind it. wrapped counts the records whose (offset_k - offset_{k-1}) mod 2^32 is above 255: the byte cannot hold them.
 *
 * Shape. A unit is a chunk of kChunk pairs of one buffer; which units there are follows from capacityPairs alone, never from the
 * data. Three kernels, no atomics:
 *    count   a wave per unit: the unit's part - how many points it keeps, the first and the last kept offset, the last kept
 *            sample, the records wrapped inside it - tile by tile of 64 pairs (a ballot, the predecessor by a lane read);
 *    scan    a wave per entry: the parts of its units merged in order (nfc_apcm_merge is associative), which gives every unit the
 *            index of its first record and the point before it - possibly the last pair of an earlier buffer - and the entry its
 *            header and its nfcgpu_apcm_info;
 *    encode  a wave per unit: the tiles once more, every kept pair's record packed to its place in a staging area (LDS), which
 *            the wave then writes out with dword stores; the bytes of the first and the last dword that belong to a neighbour
 *            unit, to the header or to nobody are not touched (byte stores for the unit's own).
 * A record whose index is not below maxRecords - what capacity_bytes holds whole - is counted and not written. A count above
 * capacityPairs is read as capacityPairs and raises the flag.
 */
#ifndef NFC_APCM_HPP
#define NFC_APCM_HPP

#include <stdint.h>

#include "nfc_record.hpp"

#define NFC_APCM_FN NFC_RECORD_FN

#define NFC_APCM_HEADER_BYTES 32u
#define NFC_APCM_MAGIC 0x4D435041u /* "APCM", little-endian */
#define NFC_APCM_VERSION 2u

struct NfcApcmShape
{
   static constexpr uint32_t kChunk = 1024;                         /* pairs of a unit */
   static constexpr uint32_t kWaves = 4;                            /* of a workgroup; each on a unit of its own */
   static constexpr uint32_t kStageDwords = kChunk * 3 / 4 + 2;     /* a unit's records behind up to three bytes of lead */
};

/* nfcgpu_apcm_info */
struct NfcApcmInfo
{
   uint32_t bytes, records, wrapped, reserved;
};

/* a control point as the resampler leaves it */
struct __attribute__((aligned(8))) NfcApcmPair
{
   float value, offset;
};

struct NfcApcmPoint
{
   uint32_t offset;
   int32_t sample;
   uint32_t keep;
};

/* what a run of consecutive points of an entry is to the points around it; has == 0: it keeps nothing */
struct NfcApcmPart
{
   uint32_t kept, wrapped;
   uint32_t first, last; /* offsets of the first and the last kept point */
   int32_t sample;       /* of the last kept point */
   uint32_t has;
};

/* what a unit starts from: the index of its first record in the entry and the point before it */
struct NfcApcmBase
{
   uint32_t record;
   uint32_t prevOffset;
   int32_t prevSample;
   uint32_t pad;
};

struct NfcApcmArgs
{
   const uint8_t *pairs;      /* buffer b at b * pairsPitch */
   const uint32_t *counts;    /* [nBuffers] */
   uint8_t *out;              /* entry e at e * outPitch */
   NfcApcmInfo *info;         /* [nEntries] */
   NfcApcmPart *parts;        /* [units] */
   NfcApcmBase *bases;        /* [units] */
   uint32_t *flag;            /* set when a count is above capacityPairs */
   uint64_t pairsPitch, outPitch; /* bytes */
   uint64_t units;            /* nBuffers * chunksPerBuffer */
   uint64_t unitsPerEntry;    /* buffersPerEntry * chunksPerBuffer */
   uint32_t nBuffers, nEntries;
   uint32_t capacityPairs, chunksPerBuffer;
   uint32_t buffersPerEntry, bufferSamples;
   uint32_t firstPosition, firstStreamId;
   uint32_t sampleRate;
   uint32_t sampleStart, sampleEnd;
   uint32_t maxRecords;       /* (capacity_bytes - 32) / 3 */
};

/* static_cast<unsigned int>(float) where the reference's is defined; 0 below and for a NaN, 2^32 - 1 above */
NFC_APCM_FN uint32_t nfc_apcm_offset(float v)
{
   if (!(v >= 1.0f))
      return 0u;
   if (v >= 4294967296.0f)
      return 0xFFFFFFFFu;
   return (uint32_t)v;
}

NFC_APCM_FN NfcApcmPart nfc_apcm_none()
{
   NfcApcmPart p;
   p.kept = 0;
   p.wrapped = 0;
   p.first = 0;
   p.last = 0;
   p.sample = 0;
   p.has = 0;
   return p;
}

/* what an entry starts from (:953-954): no record yet, the point before the first one is (sampleStart, 0) */
NFC_APCM_FN NfcApcmPart nfc_apcm_start(const NfcApcmArgs &A)
{
   NfcApcmPart p = nfc_apcm_none();
   p.first = A.sampleStart;
   p.last = A.sampleStart;
   p.has = 1;
   return p;
}

NFC_APCM_FN uint32_t nfc_apcm_wraps(uint32_t offset, uint32_t before)
{
   return (uint32_t)(offset - before) > 255u ? 1u : 0u;
}

/* the run a followed by the run b */
NFC_APCM_FN NfcApcmPart nfc_apcm_merge(const NfcApcmPart &a, const NfcApcmPart &b)
{
   NfcApcmPart r;

   r.kept = a.kept + b.kept;
   r.wrapped = a.wrapped + b.wrapped + ((a.has && b.has) ? nfc_apcm_wraps(b.first, a.last) : 0u);
   r.first = a.has ? a.first : b.first;
   r.last = b.has ? b.last : a.last;
   r.sample = b.has ? b.sample : a.sample;
   r.has = a.has | b.has;
   return r;
}

/* the run that is one kept point */
NFC_APCM_FN NfcApcmPart nfc_apcm_single(const NfcApcmPoint &p)
{
   NfcApcmPart r;

   r.kept = 1;
   r.wrapped = 0;
   r.first = p.offset;
   r.last = p.offset;
   r.sample = p.sample;
   r.has = 1;
   return r;
}

/* Unit `unit`: its buffer, the pairs begin ... end - 1 it takes of it and the buffer's stream position. Nothing beyond
 * capacityPairs is ever taken. */
NFC_APCM_FN void nfc_apcm_unit(const NfcApcmArgs &A, uint64_t unit, uint32_t &buffer, uint32_t &begin, uint32_t &end, uint32_t &position)
{
   buffer = (uint32_t)(unit / A.chunksPerBuffer);

   const uint64_t at = (unit % A.chunksPerBuffer) * NfcApcmShape::kChunk;
   uint32_t count = A.counts[buffer];

   if (count > A.capacityPairs)
   {
      count = A.capacityPairs;
      *A.flag = 1u;
   }

   begin = at < count ? (uint32_t)at : count;
   end = count - begin < NfcApcmShape::kChunk ? count : begin + NfcApcmShape::kChunk;
   position = A.firstPosition + (buffer % A.buffersPerEntry) * A.bufferSamples;
}

/* pair i (below the buffer's count) of the buffer whose row starts at `row` */
NFC_APCM_FN NfcApcmPoint nfc_apcm_point(const NfcApcmArgs &A, const NfcApcmPair *row, uint32_t position, uint32_t i)
{
   const NfcApcmPair pair = row[i];
   uint32_t clipped = 0;
   NfcApcmPoint p;

   p.offset = position + nfc_apcm_offset(pair.offset);
   p.sample = nfc_record_quantise(pair.value, clipped);
   p.keep = (p.offset >= A.sampleStart && p.offset <= A.sampleEnd) ? 1u : 0u;
   return p;
}

NFC_APCM_FN const NfcApcmPair *nfc_apcm_row(const NfcApcmArgs &A, uint32_t buffer)
{
   return reinterpret_cast<const NfcApcmPair *>(A.pairs + (uint64_t)buffer * A.pairsPitch);
}

/* the three bytes of a record, the first in the low byte */
NFC_APCM_FN uint32_t nfc_apcm_record(const NfcApcmPoint &p, uint32_t prevOffset, int32_t prevSample)
{
   return ((p.offset - prevOffset) & 0xFFu) | (((uint32_t)(p.sample - prevSample) & 0xFFFFu) << 8);
}

/* The records of a unit that are written, given where it starts: first ... last - 1 of the entry. `lead` is the byte within its
 * dword at which record `first` starts (entries and their pitch are multiples of 4, the header is 32 bytes). */
NFC_APCM_FN void nfc_apcm_window(const NfcApcmArgs &A, uint32_t record, uint32_t kept, uint32_t &first, uint32_t &last, uint32_t &lead)
{
   first = record < A.maxRecords ? record : A.maxRecords;
   last = kept < A.maxRecords - first ? first + kept : A.maxRecords;
   lead = (3u * first) & 3u;
}

/* record `rel` of the unit's window into the staging area */
NFC_APCM_FN void nfc_apcm_stage(uint32_t *stage, uint32_t lead, uint32_t rel, uint32_t record)
{
   uint8_t *at = reinterpret_cast<uint8_t *>(stage) + lead + 3u * rel;

   at[0] = (uint8_t)record;
   at[1] = (uint8_t)(record >> 8);
   at[2] = (uint8_t)(record >> 16);
}

/* Lane `lane` of the wave that writes a staging area out: bytes lead ... lead + bytes - 1 of `stage` to the same bytes of `to`,
 * which is the dword-aligned address `lead` bytes ahead of the window's first record. Whole dwords go as dwords; what the
 * window holds of its first and of its last dword goes byte by byte, so that no byte outside it is written. */
NFC_APCM_FN void nfc_apcm_flush(uint8_t *to, const uint32_t *stage, uint32_t lead, uint32_t bytes, uint32_t lane)
{
   const uint32_t span = lead + bytes;
   const uint32_t dwords = span / 4u;
   const uint8_t *from = reinterpret_cast<const uint8_t *>(stage);

   for (uint32_t j = lane; j < dwords; j += 64u)
   {
      if (j == 0 && lead)
      {
         for (uint32_t k = lead; k < 4u; k++)
            to[k] = from[k];
      }
      else
         *reinterpret_cast<uint32_t *>(to + 4u * j) = stage[j];
   }

   if (lane == (dwords & 63u))
   {
      for (uint32_t k = dwords * 4u < lead ? lead : dwords * 4u; k < span; k++)
         to[k] = from[k];
   }
}

/* where the window of an entry's unit starts in memory, `lead` bytes back */
NFC_APCM_FN uint8_t *nfc_apcm_window_at(const NfcApcmArgs &A, uint32_t entry, uint32_t first, uint32_t lead)
{
   return A.out + (uint64_t)entry * A.outPitch + NFC_APCM_HEADER_BYTES + 3ull * first - lead;
}

/* an entry whose units are all in `total` (nfc_apcm_start first): its header and its record of results */
NFC_APCM_FN void nfc_apcm_finish(const NfcApcmArgs &A, uint32_t entry, const NfcApcmPart &total)
{
   uint32_t *h = reinterpret_cast<uint32_t *>(A.out + (uint64_t)entry * A.outPitch);

   h[0] = NFC_APCM_MAGIC;
   h[1] = NFC_APCM_VERSION;
   h[2] = 0;
   h[3] = 0;
   h[4] = total.kept < A.maxRecords ? total.kept : A.maxRecords; /* the records that are there */
   h[5] = A.firstStreamId + entry;
   h[6] = A.sampleRate;
   h[7] = 0;

   NfcApcmInfo info;

   info.bytes = NFC_APCM_HEADER_BYTES + 3u * total.kept;
   info.records = total.kept;
   info.wrapped = total.wrapped;
   info.reserved = 0;
   A.info[entry] = info;
}

#endif
