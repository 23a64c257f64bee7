/*
 * nfc_tap.hpp - nfcgpu_signal_tap, held once: what the decoder's front end (NfcDecoderStatus::nextSample, NfcTech.cpp:28-105)
 * makes of every sample - the sample, the DC-removed signal, the mean deviation, the average, the envelope and the modulation
 * depth - as planes of floats. The device kernels (nfc_tap.hip) and their CPU twins of the emulated test build (nfcgpu.hip,
 * NFCGPU_EMULATED_TEST_BUILD) compile this text, as with nfc_record.hpp. The arithmetic is not here: a sample goes through
 * nfc_front_end_core of nfc_core.hpp, the decoder's own, and the one statement nfc_front_end adds for the depth.
 *
 * Shape. A buffer is cut into chunks of `chunk` samples; a walker takes one chunk, sample by sample, and a wave takes 64
 * walkers, one per lane. Memory is touched by the wave, never by a lane at a chunk's stride: for a tile of kTile samples of
 * each of its walkers the wave fetches the 64 runs of kTile samples (a run is contiguous: a load instruction takes four of
 * them), puts them into LDS, every lane walks its own row of the tile and leaves a row per selected plane, and the wave
 * writes those out the way it fetched. Rows are kRow = kTile + 1 floats apart, so the lanes of a wave meet different banks.
 *
 * Cut in time, exact all the same. Chunk 0 of a buffer starts from the state the caller gives. Every other chunk starts
 * `warm` samples early from a guessed state (nfc_tap_begin); where its warm-up reaches back to the buffer's first sample it
 * starts there from the caller's state instead. A walker notes the state it had before its chunk's first sample (starts[])
 * and after its last (ends[]). nfc_tap_seam_differs compares starts[k] with ends[k - 1] in every bit of all six fields; per
 * buffer the first chunk that differs behind chunks that are all true is walked again from ends[k - 1], without warm-up,
 * round after round until none is left. The envelope tracker is not contractive (nfc_core.hpp: nfc_envelope_step), so a
 * warm-up proves nothing by its length: only the comparison does.
 */
#ifndef NFC_TAP_HPP
#define NFC_TAP_HPP

#include <stdint.h>

#include "nfc_types.h"
#include "nfc_sample.hpp"

/* the planes, in the order they are written (NFCGPU_TAP_* of include/nfcgpu.h) */
#define NFC_TAP_VALUE 0x01u
#define NFC_TAP_FILTERED 0x02u
#define NFC_TAP_DEVIATION 0x04u
#define NFC_TAP_AVERAGE 0x08u
#define NFC_TAP_ENVELOPE 0x10u
#define NFC_TAP_DEPTH 0x20u
#define NFC_TAP_ALL 0x3Fu

struct NfcTapShape
{
   static constexpr uint32_t kWalkers = 64;                /* a wave */
   static constexpr uint32_t kTile = 16;                   /* samples of a walker per trip through LDS */
   static constexpr uint32_t kRow = kTile + 1;
   static constexpr uint32_t kRuns = 64 / kTile;           /* runs a load or store instruction of the wave takes */
   static constexpr uint32_t kPlanes = 6;
   static constexpr uint32_t kPlaneFloats = kWalkers * kRow;
};

/* what the front end carries from one sample to the next: the first six fields of NfcStreamState, in its order */
struct NfcTapState
{
   uint32_t clock, pulseFilter;
   float env, n1, mdev, avg;
};

/* nfcgpu_tap_state */
struct NfcTapRecord
{
   NfcTapState s;
   uint32_t reserved[2];
};

/* a walker's run: the samples first ... first + total - 1 of its row, of which the first `warm` are not written */
struct NfcTapWalker
{
   uint64_t inRow, outRow;   /* bytes from A.in / A.out to the buffer's row */
   uint32_t id;              /* buffer * chunksPerBuffer + chunk */
   uint32_t first, warm, total;
};

struct NfcTapArgs
{
   const uint8_t *in;
   float *out;
   const NfcTapRecord *stateIn;  /* [nBuffers], or null: every buffer a stream just opened */
   NfcTapRecord *stateOut;       /* [nBuffers], or null */
   NfcTapState *starts, *ends;   /* [nBuffers * chunksPerBuffer] */
   const uint32_t *list;         /* the ids of the walkers of a round of second walks; null: the first walk, every chunk */
   uint32_t *listOut;            /* seam kernels: the list they make, its length in count[0] */
   uint32_t *count;
   uint32_t *frontier, *next;    /* [nBuffers]: chunks that are true; the first chunk found to differ at or behind them */
   uint64_t inPitch, outPitch, planePitch; /* bytes */
   uint64_t walkers;             /* chunks in all, or the length of `list` */
   uint32_t n;                   /* samples per buffer */
   uint32_t nBuffers;
   uint32_t chunk, warm;
   uint32_t chunksPerBuffer;
   uint32_t tiles;               /* trips through LDS that cover the longest run of the launch */
   uint32_t layout;              /* nfc_sample.hpp */
   uint32_t mask;                /* NFC_TAP_* */
};

NFC_SAMPLE_FN uint32_t nfc_tap_planes(uint32_t mask)
{
   uint32_t k = 0;
   for (uint32_t bit = 0; bit < NfcTapShape::kPlanes; bit++)
      k += (mask >> bit) & 1u;
   return k;
}

/* the rest needs the decoder's step machine: nfc_core.hpp, included by whoever compiles kernels or their twins */
#ifdef NFC_AMD_CORE_HPP

/* a stream just opened: what nfc_state_init leaves */
NFC_DEV NfcTapState nfc_tap_fresh()
{
   NfcTapState s;
   s.clock = 0xFFFFFFFFu;
   s.pulseFilter = 0;
   s.env = 0; s.n1 = 0; s.mdev = 0; s.avg = 0;
   return s;
}

/* walker `slot` of the launch; total == 0: there is none */
NFC_DEV NfcTapWalker nfc_tap_walker(const NfcTapArgs &A, uint64_t slot)
{
   NfcTapWalker w;
   w.inRow = 0; w.outRow = 0; w.id = 0; w.first = 0; w.warm = 0; w.total = 0;

   if (slot >= A.walkers)
      return w;

   w.id = A.list ? A.list[slot] : (uint32_t)slot;

   const uint32_t b = w.id / A.chunksPerBuffer, k = w.id % A.chunksPerBuffer;
   const uint64_t begin = (uint64_t)k * A.chunk;
   const uint64_t left = A.n - begin;
   const uint32_t len = left < A.chunk ? (uint32_t)left : A.chunk;

   w.warm = A.list ? 0u : (uint32_t)(begin < A.warm ? begin : A.warm);
   w.first = (uint32_t)begin - w.warm;
   w.total = w.warm + len;
   w.inRow = (uint64_t)b * A.inPitch;
   w.outRow = (uint64_t)b * A.outPitch;
   return w;
}

/* The state a walker has before the sample `first`. A second walk starts where the chunk before ended; a run that begins with
 * its buffer starts from the caller's state; anything else is a guess - a carrier at the level of the first sample, tracked,
 * the filter settled on it, no deviation - with the one thing that is known, the clock. Nothing depends on the guess but how
 * many chunks are walked twice. */
NFC_DEV NfcTapState nfc_tap_begin(const NfcTapArgs &A, const NfcTapWalker &w)
{
   if (A.list)
      return A.ends[w.id - 1u];

   NfcTapState s = A.stateIn ? A.stateIn[w.id / A.chunksPerBuffer].s : nfc_tap_fresh();

   if (w.first == 0)
      return s;

   const float x = nfc_sample_at(A.in + w.inRow, A.layout, w.first);

   s.clock = s.clock + w.first;
   s.pulseFilter = 0;
   s.env = x;
   s.n1 = x * 10.0f;
   s.mdev = 0;
   s.avg = x;
   return s;
}

/* One sample: ++clock, ++pulseFilter, nfc_front_end_core, and the depth as nfc_front_end forms it (nfc_core.hpp:408-411).
 * v[] takes the six values in plane order. Of NfcStreamState only the front end's fields exist here; the edge tracker runs on
 * two that nobody reads. */
NFC_DEV void nfc_tap_sample(const NfcConfig &c, NfcTapState &t, float value, float v[NfcTapShape::kPlanes])
{
   NfcStreamState s;

   s.clock = t.clock + 1u;
   s.pulseFilter = t.pulseFilter + 1u;
   s.env = t.env; s.n1 = t.n1; s.mdev = t.mdev; s.avg = t.avg;
   s.edgePeak = 0; s.edgeTime = 0;

   const NfcNow now = nfc_front_end_core(c, s, value);

   const float env = s.env;
   const float clamped = (value < 0.0f) ? 0.0f : ((env < value) ? env : value);

   v[0] = now.x;
   v[1] = now.filt;
   v[2] = now.mdev;
   v[3] = s.avg;
   v[4] = env;
   v[5] = (env - clamped) / env;

   t.clock = s.clock;
   t.pulseFilter = s.pulseFilter;
   t.env = s.env; t.n1 = s.n1; t.mdev = s.mdev; t.avg = s.avg;
}

/* Lane `lane` of the wave fetches its share of tile `tile`: of each of the wave's walkers kTile samples, run by run. */
NFC_DEV void nfc_tap_fetch(const NfcTapArgs &A, const NfcTapWalker *walkers, uint32_t tile, uint32_t lane, float *tileIn)
{
   const uint32_t col = lane % NfcTapShape::kTile;
   const uint32_t p = tile * NfcTapShape::kTile + col;

   for (uint32_t r = 0; r < NfcTapShape::kTile; r++)
   {
      const uint32_t j = r * NfcTapShape::kRuns + lane / NfcTapShape::kTile;
      const NfcTapWalker &w = walkers[j];

      if (p < w.total)
         tileIn[j * NfcTapShape::kRow + col] = nfc_sample_at(A.in + w.inRow, A.layout, w.first + p);
   }
}

/* Lane `lane` walks its row of the tile; `start` takes the state before the chunk's first sample when the tile holds it. */
NFC_DEV void nfc_tap_walk(const NfcTapArgs &A, const NfcConfig &c, const NfcTapWalker &w, uint32_t tile, uint32_t lane, NfcTapState &s,
                          NfcTapState &start, const float *tileIn, float *tileOut)
{
   for (uint32_t i = 0; i < NfcTapShape::kTile; i++)
   {
      const uint32_t p = tile * NfcTapShape::kTile + i;

      if (p < w.total)
      {
         if (p == w.warm)
            start = s;

         float v[NfcTapShape::kPlanes];
         nfc_tap_sample(c, s, tileIn[lane * NfcTapShape::kRow + i], v);

         uint32_t k = 0;
         for (uint32_t bit = 0; bit < NfcTapShape::kPlanes; bit++)
         {
            if ((A.mask >> bit) & 1u)
            {
               tileOut[k * NfcTapShape::kPlaneFloats + lane * NfcTapShape::kRow + i] = v[bit];
               k++;
            }
         }
      }
   }
}

/* Lane `lane` writes its share of what the wave's walkers left of tile `tile`, but for the warm-ups. */
NFC_DEV void nfc_tap_store(const NfcTapArgs &A, const NfcTapWalker *walkers, uint32_t tile, uint32_t lane, uint32_t planes, const float *tileOut)
{
   const uint32_t col = lane % NfcTapShape::kTile;
   const uint32_t p = tile * NfcTapShape::kTile + col;

   for (uint32_t r = 0; r < NfcTapShape::kTile; r++)
   {
      const uint32_t j = r * NfcTapShape::kRuns + lane / NfcTapShape::kTile;
      const NfcTapWalker &w = walkers[j];

      if (p >= w.warm && p < w.total)
      {
         uint8_t *at = reinterpret_cast<uint8_t *>(A.out) + w.outRow + (uint64_t)(w.first + p) * 4u;

         for (uint32_t k = 0; k < planes; k++)
            *reinterpret_cast<float *>(at + k * A.planePitch) = tileOut[k * NfcTapShape::kPlaneFloats + j * NfcTapShape::kRow + col];
      }
   }
}

/* what a walker leaves behind its run */
NFC_DEV void nfc_tap_end(const NfcTapArgs &A, const NfcTapWalker &w, const NfcTapState &start, const NfcTapState &end)
{
   if (w.total)
   {
      A.starts[w.id] = start;
      A.ends[w.id] = end;
   }
}

/* every bit of all six fields */
NFC_DEV bool nfc_tap_seam_differs(const NfcTapState &a, const NfcTapState &b)
{
   return ((a.clock ^ b.clock) | (a.pulseFilter ^ b.pulseFilter) | (nfc_bits(a.env) ^ nfc_bits(b.env)) | (nfc_bits(a.n1) ^ nfc_bits(b.n1)) |
           (nfc_bits(a.mdev) ^ nfc_bits(b.mdev)) | (nfc_bits(a.avg) ^ nfc_bits(b.avg))) != 0;
}

/* chunk `id` (not a buffer's first) keeps its buffer from being true up to here: it lies at or behind the buffer's frontier and
 * did not start where the chunk before ended */
NFC_DEV bool nfc_tap_seam_open(const NfcTapArgs &A, uint32_t id)
{
   const uint32_t b = id / A.chunksPerBuffer, k = id % A.chunksPerBuffer;

   return k != 0 && k >= A.frontier[b] && nfc_tap_seam_differs(A.starts[id], A.ends[id - 1u]);
}

/* buffer b once its chunks have been looked at: the frontier moves to the first open seam, which is listed; true: there is one */
NFC_DEV bool nfc_tap_seam_close(const NfcTapArgs &A, uint32_t b, uint32_t &id)
{
   const uint32_t k = A.next[b] < A.chunksPerBuffer ? A.next[b] : A.chunksPerBuffer; /* (0xFFFFFFFF: none was found) */

   A.frontier[b] = k;
   A.next[b] = 0xFFFFFFFFu;
   id = b * A.chunksPerBuffer + k;
   return k < A.chunksPerBuffer;
}

/* the state behind a buffer's last sample */
NFC_DEV void nfc_tap_finish(const NfcTapArgs &A, uint32_t b)
{
   NfcTapRecord r;
   r.s = A.ends[(uint64_t)b * A.chunksPerBuffer + A.chunksPerBuffer - 1u];
   r.reserved[0] = 0;
   r.reserved[1] = 0;
   A.stateOut[b] = r;
}

#endif

#endif
