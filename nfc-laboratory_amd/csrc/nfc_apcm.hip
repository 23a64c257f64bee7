/*
 * nfc_apcm.hip - device kernels of nfcgpu_apcm_encode: the resampler's control points delta-coded into APCM entries. What a point,
 * a part, a record and a unit's window are, and how a staging area is written out, is nfc_apcm.hpp; this file adds the grids, the
 * ballots and the scan over a wave.
 *
 * nfc_apcm_count_kernel: a wave per unit, grid-stride, four waves to a workgroup that share nothing. A tile is 64 consecutive
 * pairs, one 8-byte load per lane; the ballot of the kept ones gives their number, the lane below a kept lane that is kept too
 * gives its predecessor. nfc_apcm_scan_kernel: a wave per entry scans the parts of its units, 64 at a time, with nfc_apcm_merge.
 * nfc_apcm_encode_kernel: the tiles again; a kept lane packs its record into the wave's staging area in LDS, the wave writes the
 * area out (nfc_apcm_flush). The loops over the units are the same length for the four waves of a workgroup, so that they meet
 * at the barriers around the staging area. No atomics: an entry has the same bytes on every run.
 */
#include <hip/hip_runtime.h>

#include "nfc_apcm.hpp"

namespace {

__device__ __forceinline__ uint32_t nfc_apcm_highest(uint64_t mask)
{
   return 63u - (uint32_t)__builtin_clzll(mask);
}

/* One tile of a unit: the point of every lane (keep == 0 where there is none), and for the kept lanes the point before them -
 * of the tile, or what `run` ends with (hasBefore: is there one at all). `run` then takes the tile in. All lanes of the wave
 * call this together; mask and run are the same in all of them. */
__device__ __forceinline__ uint64_t nfc_apcm_tile(const NfcApcmArgs &A, const NfcApcmPair *row, uint32_t position, uint32_t i, uint32_t end, uint32_t lane,
                                                  NfcApcmPart &run, NfcApcmPoint &p, uint32_t &beforeOffset, int32_t &beforeSample, uint32_t &hasBefore,
                                                  uint32_t &rank)
{
   p.offset = 0;
   p.sample = 0;
   p.keep = 0;

   if (i < end)
      p = nfc_apcm_point(A, row, position, i);

   const uint64_t mask = __ballot(p.keep != 0);
   const uint64_t below = mask & ((1ull << lane) - 1ull);
   const uint32_t from = below ? nfc_apcm_highest(below) : lane;
   const uint32_t tileOffset = __shfl(p.offset, (int)from);
   const int32_t tileSample = __shfl(p.sample, (int)from);

   beforeOffset = below ? tileOffset : run.last;
   beforeSample = below ? tileSample : run.sample;
   hasBefore = below ? 1u : run.has;
   rank = (uint32_t)__popcll(below);

   if (mask)
   {
      const uint64_t wrapped = __ballot(p.keep && hasBefore && nfc_apcm_wraps(p.offset, beforeOffset));
      const uint32_t firstLane = (uint32_t)__builtin_ctzll(mask), lastLane = nfc_apcm_highest(mask);
      const uint32_t firstOffset = __shfl(p.offset, (int)firstLane);

      if (!run.has)
         run.first = firstOffset;
      run.last = __shfl(p.offset, (int)lastLane);
      run.sample = __shfl(p.sample, (int)lastLane);
      run.has = 1;
      run.kept += (uint32_t)__popcll(mask);
      run.wrapped += (uint32_t)__popcll(wrapped);
   }

   return mask;
}

__device__ __forceinline__ NfcApcmPart nfc_apcm_shfl_up(const NfcApcmPart &x, uint32_t off)
{
   NfcApcmPart y;
   y.kept = __shfl_up(x.kept, off);
   y.wrapped = __shfl_up(x.wrapped, off);
   y.first = __shfl_up(x.first, off);
   y.last = __shfl_up(x.last, off);
   y.sample = __shfl_up(x.sample, off);
   y.has = __shfl_up(x.has, off);
   return y;
}

__device__ __forceinline__ NfcApcmPart nfc_apcm_of_lane(const NfcApcmPart &x, int lane)
{
   NfcApcmPart y;
   y.kept = __shfl(x.kept, lane);
   y.wrapped = __shfl(x.wrapped, lane);
   y.first = __shfl(x.first, lane);
   y.last = __shfl(x.last, lane);
   y.sample = __shfl(x.sample, lane);
   y.has = __shfl(x.has, lane);
   return y;
}

}

__global__ __launch_bounds__(64 * NfcApcmShape::kWaves) void nfc_apcm_count_kernel(NfcApcmArgs A)
{
   const uint32_t lane = threadIdx.x & 63u;
   const uint64_t waves = (uint64_t)gridDim.x * NfcApcmShape::kWaves;

   for (uint64_t unit = (uint64_t)blockIdx.x * NfcApcmShape::kWaves + (threadIdx.x >> 6); unit < A.units; unit += waves)
   {
      uint32_t buffer, begin, end, position;

      nfc_apcm_unit(A, unit, buffer, begin, end, position);

      const NfcApcmPair *row = nfc_apcm_row(A, buffer);
      NfcApcmPart run = nfc_apcm_none();

      for (uint32_t base = begin; base < end; base += 64u)
      {
         NfcApcmPoint p;
         uint32_t beforeOffset, hasBefore, rank;
         int32_t beforeSample;

         nfc_apcm_tile(A, row, position, base + lane, end, lane, run, p, beforeOffset, beforeSample, hasBefore, rank);
      }

      if (lane == 0)
         A.parts[unit] = run;
   }
}

__global__ __launch_bounds__(64) void nfc_apcm_scan_kernel(NfcApcmArgs A)
{
   const uint32_t lane = threadIdx.x & 63u;

   for (uint32_t entry = blockIdx.x; entry < A.nEntries; entry += gridDim.x)
   {
      const uint64_t first = (uint64_t)entry * A.unitsPerEntry;
      NfcApcmPart carry = nfc_apcm_start(A);

      for (uint64_t base = 0; base < A.unitsPerEntry; base += 64u)
      {
         const bool there = base + lane < A.unitsPerEntry;
         NfcApcmPart x = there ? A.parts[first + base + lane] : nfc_apcm_none();

         /* x: the units base ... base + lane of the entry */
         for (uint32_t off = 1; off < 64u; off <<= 1)
         {
            const NfcApcmPart y = nfc_apcm_shfl_up(x, off);

            if (lane >= off)
               x = nfc_apcm_merge(y, x);
         }

         const NfcApcmPart upTo = nfc_apcm_shfl_up(x, 1);
         const NfcApcmPart before = lane ? nfc_apcm_merge(carry, upTo) : carry;

         if (there)
         {
            NfcApcmBase b;

            b.record = before.kept;
            b.prevOffset = before.last;
            b.prevSample = before.sample;
            b.pad = 0;
            A.bases[first + base + lane] = b;
         }

         carry = nfc_apcm_merge(carry, nfc_apcm_of_lane(x, 63));
      }

      if (lane == 0)
         nfc_apcm_finish(A, entry, carry);
   }
}

__global__ __launch_bounds__(64 * NfcApcmShape::kWaves) void nfc_apcm_encode_kernel(NfcApcmArgs A)
{
   __shared__ uint32_t stages[NfcApcmShape::kWaves][NfcApcmShape::kStageDwords];

   const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
   const uint64_t waves = (uint64_t)gridDim.x * NfcApcmShape::kWaves;
   uint32_t *stage = stages[wave];

   /* (the same trips for every wave of the workgroup: the barriers) */
   for (uint64_t head = (uint64_t)blockIdx.x * NfcApcmShape::kWaves; head < A.units; head += waves)
   {
      const uint64_t unit = head + wave;
      const bool there = unit < A.units;
      const uint32_t kept = there ? A.parts[unit].kept : 0u;
      uint32_t first = 0, last = 0, lead = 0, entry = 0;

      if (kept)
      {
         const NfcApcmBase b = A.bases[unit];
         uint32_t buffer, begin, end, position;

         nfc_apcm_unit(A, unit, buffer, begin, end, position);
         nfc_apcm_window(A, b.record, kept, first, last, lead);
         entry = buffer / A.buffersPerEntry;

         const NfcApcmPair *row = nfc_apcm_row(A, buffer);
         NfcApcmPart run = nfc_apcm_none();
         uint32_t done = 0;

         run.last = b.prevOffset;
         run.sample = b.prevSample;
         run.has = 1;

         for (uint32_t base = begin; base < end && first + done < last; base += 64u)
         {
            NfcApcmPoint p;
            uint32_t beforeOffset, hasBefore, rank;
            int32_t beforeSample;

            const uint64_t mask = nfc_apcm_tile(A, row, position, base + lane, end, lane, run, p, beforeOffset, beforeSample, hasBefore, rank);

            /* (first + rel < last <= first + kept: rel is below kChunk) */
            const uint32_t rel = done + rank;

            if (p.keep && first + rel < last)
               nfc_apcm_stage(stage, lead, rel, nfc_apcm_record(p, beforeOffset, beforeSample));

            done += (uint32_t)__popcll(mask);
         }
      }

      __syncthreads();

      if (last > first)
         nfc_apcm_flush(nfc_apcm_window_at(A, entry, first, lead), stage, lead, 3u * (last - first), lane);

      __syncthreads();
   }
}
