/*
 * nfcgpu.hip — host runtime behind the C ABI of include/nfcgpu.h.
 *
 * Owns, per context: one HIP stream, the HBM-resident stream slots (state records, history rings,
 * frame assembly buffers), the device frame sink and the per-stream host frame queues. Streams are
 * grouped into stream blocks of 64 (one wavefront). There is deliberately no CPU decoding path here:
 * if HIP or the gfx950 code object is unavailable every entry point fails with NFCGPU_ENODEV/EHIP.
 */
#include <hip/hip_runtime.h>

#include <dlfcn.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <algorithm>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/nfcgpu.h"
#include "nfc_config.hpp"
#include "nfc_launch.h"
#include "nfc_scan_launch.h"
#include "nfc_spectrum.hpp"
#include "nfc_sample.hpp"
#include "nfc_record.hpp"
#include "nfc_resample.hpp"
#ifdef NFCGPU_EMULATED_TEST_BUILD
/* (the twins of the tap kernels walk the decoder's step machine: nfc_core.hpp as the CPU builds of tests/hostsim compile it) */
#define NFC_DEV static inline
static inline uint32_t tap_twin_add(uint32_t *p, uint32_t v) { const uint32_t old = *p; *p += v; return old; }
#define NFC_ATOMIC_ADD(ptr, value) tap_twin_add((ptr), (value))
#define NFC_ANY(predicate) (predicate)
#include "nfc_core.hpp"
#endif
#include "nfc_tap.hpp"
#include "nfc_tap_reduce.hpp"
#include "nfc_apcm.hpp"

__global__ void nfc_demod_kernel(const NfcConfig *__restrict__ cfgPtr, NfcLaunch L);
__global__ void nfc_demod_exact_kernel(const NfcConfig *__restrict__ cfgPtr, NfcLaunch L);
__global__ void nfc_magnitude_kernel(const float2 *__restrict__ iq, float *__restrict__ out, uint64_t n);
__global__ void nfc_resample_radio_kernel(const float *__restrict__ in, uint64_t pitchFloats, uint32_t nBuffers, uint32_t n,
                                          float *__restrict__ out, uint64_t outPitchFloats, uint32_t capacityPairs,
                                          uint32_t *__restrict__ counts);
__global__ void nfc_demod_fixed_kernel(const NfcConfig *__restrict__ cfgPtr, NfcLaunch L);
__global__ void nfc_demod_fixed_exact_kernel(const NfcConfig *__restrict__ cfgPtr, NfcLaunch L);

/* the table the specialised kernels were compiled with (generated at build time, see gen_fixed_config.cpp) */
#define NFC_FIXED_FN static inline
#include "nfc_config_fixed.inc"
__global__ void nfc_init_kernel(const NfcConfig *__restrict__ cfgPtr, NfcLaunch L, uint32_t keepFrontEnd);
__global__ void nfc_scan_kernel(const NfcConfig *__restrict__ cfgPtr, NfcScanArgs A);
__global__ void nfc_seams_kernel(NfcScanArgs A, uint32_t first);
__global__ void nfc_tiles_kernel(const NfcConfig *__restrict__ cfgPtr, NfcScanArgs A, uint32_t nTilesTotal);
__global__ void nfc_windows_kernel(NfcScanArgs A);
__global__ void nfc_carry_lanes_kernel(NfcScanArgs A, NfcLaunch real, NfcLaunch lanes, uint32_t pass);
__global__ void nfc_window_lanes_kernel(const NfcConfig *__restrict__ cfgPtr, NfcScanArgs A, NfcLaunch lanes, uint32_t pass, uint32_t order, uint32_t lenLo, uint32_t lenHi);
__global__ void nfc_final_lanes_kernel(const NfcConfig *__restrict__ cfgPtr, NfcScanArgs A, NfcLaunch lanes);
__global__ void nfc_chain_kernel(NfcScanArgs A, NfcLaunch lanes, uint32_t maxPasses);
__global__ void nfc_finish_kernel(NfcScanArgs A, NfcLaunch real, NfcLaunch lanes);
__global__ void nfc_read_kernel(const float4 *__restrict__ data, uint64_t n, float *__restrict__ out);
__global__ void nfc_scan_planes_kernel(const NfcConfig *__restrict__ cfgPtr, NfcScanArgs A);
__global__ void nfc_envelope_kernel(const NfcConfig *__restrict__ cfgPtr, NfcScanArgs A);
__global__ void nfc_wave_kernel(const NfcConfig *__restrict__ cfgPtr, NfcLaunch L, NfcScanArgs A, uint32_t mode);
__global__ void nfc_planes_stale_kernel(NfcScanArgs A, const NfcScanChunk *all, uint32_t nAll, NfcScanChunk *out, uint32_t *count);

/* The kernels that read samples exist once per sample format (nfc_sample.hpp): the int16 ones are the same text compiled for
 * int16 rows, so that the float ones stay the code they were. NFC_BY_LAYOUT picks by a submission's layout. (The emulated test
 * build has twins of the float kernels only and widens int16 input before it gets here: widen_i16.) */
#ifdef NFCGPU_EMULATED_TEST_BUILD
#define NFC_BY_LAYOUT(layout, kernel) (kernel)
#else
__global__ void nfc_demod_kernel_i16(const NfcConfig *__restrict__ cfgPtr, NfcLaunch L);
__global__ void nfc_demod_exact_kernel_i16(const NfcConfig *__restrict__ cfgPtr, NfcLaunch L);
__global__ void nfc_demod_fixed_kernel_i16(const NfcConfig *__restrict__ cfgPtr, NfcLaunch L);
__global__ void nfc_demod_fixed_exact_kernel_i16(const NfcConfig *__restrict__ cfgPtr, NfcLaunch L);
__global__ void nfc_magnitude_kernel_i16(const NfcIq16 *__restrict__ iq, float *__restrict__ out, uint64_t n);
__global__ void nfc_scan_kernel_i16(const NfcConfig *__restrict__ cfgPtr, NfcScanArgs A);
__global__ void nfc_scan_planes_kernel_i16(const NfcConfig *__restrict__ cfgPtr, NfcScanArgs A);
__global__ void nfc_envelope_kernel_i16(const NfcConfig *__restrict__ cfgPtr, NfcScanArgs A);
__global__ void nfc_wave_kernel_i16(const NfcConfig *__restrict__ cfgPtr, NfcLaunch L, NfcScanArgs A, uint32_t mode);
#define NFC_BY_LAYOUT(layout, kernel) (((layout) & NFC_SAMPLE_I16) ? kernel##_i16 : kernel)
#endif

#ifdef NFCGPU_EMULATED_TEST_BUILD
/* The test build's twins of the spectrum kernels (nfc_spectrum.hip): the same steps from nfc_spectrum.hpp, the grid, the
 * steps and the threads of a workgroup as loops, the end of a loop over the threads where the device has a barrier. */
namespace {

template <int L, int STEP, bool I16>
void spectrum_twin_steps(const NfcSpectrumArgs &A, uint64_t frame, NfcSpectrumRegs<L> *regs, float *ldsRe, float *ldsIm)
{
   for (int lane = 0; lane < NfcSpectrumShape<L>::kThreads; lane++)
      nfc_spectrum_step<L, STEP, I16>(A, frame, lane, regs[lane], ldsRe, ldsIm);

   if constexpr (STEP + 1 < NfcSpectrumShape<L>::kSteps)
      spectrum_twin_steps<L, STEP + 1, I16>(A, frame, regs, ldsRe, ldsIm);
}

template <int L, bool I16>
void spectrum_twin(const NfcSpectrumArgs &A)
{
   static NfcSpectrumRegs<L> regs[NfcSpectrumShape<L>::kThreads];
   static float ldsRe[NfcSpectrumShape<L>::kLdsFloats], ldsIm[NfcSpectrumShape<L>::kLdsFloats];

   for (uint64_t block = 0; block < fakehip::launchGrid.x; block++)
      for (uint64_t frame = block; frame < A.total; frame += fakehip::launchGrid.x)
         spectrum_twin_steps<L, 0, I16>(A, frame, regs, ldsRe, ldsIm);
}

}
#define NFC_SPECTRUM_KERNEL(L) \
   void nfc_spectrum_kernel_##L(NfcSpectrumArgs A) { spectrum_twin<L, false>(A); } \
   void nfc_spectrum_kernel_i16_##L(NfcSpectrumArgs A) { spectrum_twin<L, true>(A); }
#else
#define NFC_SPECTRUM_KERNEL(L) \
   __global__ void nfc_spectrum_kernel_##L(NfcSpectrumArgs A); \
   __global__ void nfc_spectrum_kernel_i16_##L(NfcSpectrumArgs A);
#endif
NFC_SPECTRUM_KERNEL(256)
NFC_SPECTRUM_KERNEL(512)
NFC_SPECTRUM_KERNEL(1024)
NFC_SPECTRUM_KERNEL(2048)
NFC_SPECTRUM_KERNEL(4096)
#undef NFC_SPECTRUM_KERNEL

#ifdef NFCGPU_EMULATED_TEST_BUILD
/* The test build's twins of the resampler kernels of nfc_resample.hip: buffer after buffer, the tiles and the ring of
 * nfc_resample.hpp, a sample converted on its way into the ring and decided from there by the text the device compiles. (The float
 * magnitude kernel's twin is tests/hostsim/emu_kernels.cpp's, as it was.) */
namespace {

template <uint32_t LAYOUT>
void resample_twin(const NfcResampleArgs &A)
{
   using S = NfcResampleShape;

   float ring[S::kPitch];

   for (uint32_t buffer = 0; buffer < A.nBuffers; buffer++)
   {
      NfcResampleLane s;
      nfc_resample_begin(s);

      for (uint32_t base = 0; base < A.n; base += S::kTile)
      {
         for (uint32_t col = 0; col < S::kTile; col++)
            ring[(base % S::kRing) + col] = nfc_resample_sample<LAYOUT>(A, buffer, base + col);

         nfc_resample_decide(A, buffer, true, s, ring, base);
      }

      nfc_resample_end(A, buffer, true, s);
   }
}

}
#define NFC_RESAMPLE_KERNEL(name, LAYOUT) \
   void name(NfcResampleArgs A) { resample_twin<LAYOUT>(A); }
#else
#define NFC_RESAMPLE_KERNEL(name, LAYOUT) __global__ void name(NfcResampleArgs A);
#endif
NFC_RESAMPLE_KERNEL(nfc_resample_radio_kernel_i16, NFC_SAMPLE_I16 | 1u)
NFC_RESAMPLE_KERNEL(nfc_resample_radio_kernel_iq_i16, NFC_SAMPLE_I16 | 2u)
NFC_RESAMPLE_KERNEL(nfc_resample_radio_kernel_iq, 2u)
#undef NFC_RESAMPLE_KERNEL

#ifdef NFCGPU_EMULATED_TEST_BUILD
/* The test build's twins of the record kernels (nfc_record.hip): the quads, lanes, waves and segments of nfc_record.hpp as loops,
 * every sum in the order the device takes it (the butterfly over a wave included). PCM goes out sample by sample: what is
 * written does not depend on how the device packs its stores. */
namespace {

template <typename V, typename ADD>
void record_twin_butterfly(V *lanes, ADD add)
{
   for (int off = 1; off < 64; off <<= 1)
   {
      V next[64];
      for (int lane = 0; lane < 64; lane++)
         next[lane] = add(lanes[lane], lanes[lane ^ off]);
      for (int lane = 0; lane < 64; lane++)
         lanes[lane] = next[lane];
   }
}

template <int STRIDE, int MODE, bool LEVELS>
void record_twin(const NfcRecordArgs &A)
{
   constexpr uint32_t EB = 2 * NfcRecordKind<STRIDE, MODE>::kChannels, IB = 4 * STRIDE;

   for (uint64_t item = 0; item < A.total; item++)
   {
      const uint64_t b = item / A.nSegments;
      const uint32_t s = (uint32_t)(item % A.nSegments);
      const uint8_t *row = reinterpret_cast<const uint8_t *>(A.in) + b * A.inPitch;
      uint8_t *orow = reinterpret_cast<uint8_t *>(A.out) + b * A.outPitch;
      NfcRecordPartial waves[NfcRecordShape::kWaves];

      for (uint32_t wave = 0; wave < NfcRecordShape::kWaves; wave++)
      {
         const uint32_t q0 = s * NfcRecordShape::kSegmentQuads + wave * NfcRecordShape::kWaveQuads;
         NfcRecordPartial lanes[64];

         for (uint32_t lane = 0; lane < 64; lane++)
         {
            NfcRecordPartial acc;
            nfc_record_begin(acc);

            for (uint32_t t = 0; t < NfcRecordShape::kIters && (uint64_t)q0 * 4 < A.n; t++)
            {
               const uint64_t i0 = (uint64_t)(q0 + t * 64 + lane) * 4;
               const uint32_t valid = i0 < A.n ? (A.n - i0 < 4 ? (uint32_t)(A.n - i0) : 4u) : 0u;
               uint32_t e[4] = {0, 0, 0, 0};

               if (valid)
                  nfc_record_quad<STRIDE, MODE, LEVELS>(reinterpret_cast<const float *>(row + i0 * IB), valid, e, acc, A.w);
               else if (LEVELS)
                  nfc_record_quad_none(acc, A.w);

               for (uint32_t p = 0; p < valid; p++)
                  std::memcpy(orow + (i0 + p) * EB, &e[p], EB); /* (little-endian host) */
            }

            nfc_record_lane_end(acc, lane, A.w);
            lanes[lane] = acc;
         }

         if (LEVELS)
            record_twin_butterfly(lanes, [](const NfcRecordPartial &x, const NfcRecordPartial &y) { return nfc_record_add(x, y); });
         waves[wave] = lanes[0];
      }

      if (LEVELS)
         A.partials[item] = nfc_record_segment(waves, A.w);
   }
}

}

void nfc_record_finish_kernel(NfcRecordArgs A)
{
   for (uint32_t b = 0; b < A.nBuffers; b++)
   {
      const NfcRecordPartial *seg = A.partials + (uint64_t)b * A.nSegments;
      float peak = nfc_record_nan();
      uint32_t clipped = 0;
      std::vector<float> sums(A.nSegments);

      for (uint32_t s = 0; s < A.nSegments; s++)
      {
         peak = nfc_record_max(peak, seg[s].peak);
         clipped += seg[s].clipped;
         sums[s] = seg[s].power;
      }

      /* groups of 64 until one value is left, short groups filled with zeros */
      while (sums.size() > 1)
      {
         std::vector<float> next((sums.size() + 63) / 64);
         for (size_t g = 0; g < next.size(); g++)
         {
            float lanes[64];
            for (size_t lane = 0; lane < 64; lane++)
               lanes[lane] = g * 64 + lane < sums.size() ? sums[g * 64 + lane] : 0.0f;
            record_twin_butterfly(lanes, [](float x, float y) { return x + y; });
            next[g] = lanes[0];
         }
         sums.swap(next);
      }

      A.levels[b] = nfc_record_levels(sums[0], nfc_record_chain_average(seg, A.nSegments, A.w), peak, clipped, A.n);
   }
}
#define NFC_RECORD_KERNEL(name, STRIDE, MODE, LEVELS) \
   void name(NfcRecordArgs A) { record_twin<STRIDE, MODE, LEVELS>(A); }
#else
#define NFC_RECORD_KERNEL(name, STRIDE, MODE, LEVELS) __global__ void name(NfcRecordArgs A);
__global__ void nfc_record_finish_kernel(NfcRecordArgs A);
#endif
NFC_RECORD_KERNEL(nfc_record_kernel_mono, 1, NFC_RECORD_SAME, false)
NFC_RECORD_KERNEL(nfc_record_kernel_mono_levels, 1, NFC_RECORD_SAME, true)
NFC_RECORD_KERNEL(nfc_record_kernel_iq, 2, NFC_RECORD_SAME, false)
NFC_RECORD_KERNEL(nfc_record_kernel_iq_levels, 2, NFC_RECORD_SAME, true)
NFC_RECORD_KERNEL(nfc_record_kernel_magnitude, 2, NFC_RECORD_MAGNITUDE, false)
NFC_RECORD_KERNEL(nfc_record_kernel_magnitude_levels, 2, NFC_RECORD_MAGNITUDE, true)
#undef NFC_RECORD_KERNEL

#ifdef NFCGPU_EMULATED_TEST_BUILD
/* The test build's twins of the tap kernels (nfc_tap.hip): the groups, tiles and lanes of nfc_tap.hpp as loops, the end of a loop
 * over the lanes where the device has a barrier, a plain minimum where it has an atomic one. */
void nfc_tap_walk_kernel(NfcTapArgs A, NfcConfig cfg)
{
   static float tiles[(1 + NfcTapShape::kPlanes) * NfcTapShape::kPlaneFloats];
   float *tileIn = tiles, *tileOut = tiles + NfcTapShape::kPlaneFloats;
   NfcTapWalker walkers[NfcTapShape::kWalkers];
   NfcTapState s[NfcTapShape::kWalkers], start[NfcTapShape::kWalkers];

   const uint32_t planes = nfc_tap_planes(A.mask);
   const uint64_t groups = (A.walkers + NfcTapShape::kWalkers - 1) / NfcTapShape::kWalkers;

   for (uint64_t group = 0; group < groups; group++)
   {
      for (uint32_t lane = 0; lane < NfcTapShape::kWalkers; lane++)
      {
         walkers[lane] = nfc_tap_walker(A, group * NfcTapShape::kWalkers + lane);
         s[lane] = walkers[lane].total ? nfc_tap_begin(A, walkers[lane]) : nfc_tap_fresh();
         start[lane] = s[lane];
      }

      for (uint32_t tile = 0; tile < A.tiles; tile++)
      {
         for (uint32_t lane = 0; lane < NfcTapShape::kWalkers; lane++)
            nfc_tap_fetch(A, walkers, tile, lane, tileIn);
         for (uint32_t lane = 0; lane < NfcTapShape::kWalkers; lane++)
            nfc_tap_walk(A, cfg, walkers[lane], tile, lane, s[lane], start[lane], tileIn, tileOut);
         for (uint32_t lane = 0; lane < NfcTapShape::kWalkers; lane++)
            nfc_tap_store(A, walkers, tile, lane, planes, tileOut);
      }

      for (uint32_t lane = 0; lane < NfcTapShape::kWalkers; lane++)
         nfc_tap_end(A, walkers[lane], start[lane], s[lane]);
   }
}

void nfc_tap_seam_kernel(NfcTapArgs A)
{
   for (uint64_t id = 0; id < (uint64_t)A.nBuffers * A.chunksPerBuffer; id++)
   {
      uint32_t &next = A.next[id / A.chunksPerBuffer];
      const uint32_t k = (uint32_t)(id % A.chunksPerBuffer);

      if (nfc_tap_seam_open(A, (uint32_t)id) && k < next)
         next = k;
   }
}

void nfc_tap_list_kernel(NfcTapArgs A)
{
   for (uint32_t b = 0; b < A.nBuffers; b++)
   {
      uint32_t id;

      if (nfc_tap_seam_close(A, b, id))
         A.listOut[A.count[0]++] = id;
   }
}

void nfc_tap_finish_kernel(NfcTapArgs A)
{
   for (uint32_t b = 0; b < A.nBuffers; b++)
      nfc_tap_finish(A, b);
}

/* ... and of the kernels that reduce its planes (nfc_tap_reduce.hip): the units, the lanes and the butterfly of nfc_tap_reduce.hpp
 * as loops, every sum in the order the device takes it. */
void nfc_tap_reduce_kernel(NfcTapReduceArgs A)
{
   for (uint64_t j = 0; j < A.units; j++)
   {
      NfcTapPartial lanes[64];

      for (uint32_t lane = 0; lane < 64; lane++)
         lanes[lane] = nfc_tap_reduce_lane(A, j, lane);

      record_twin_butterfly(lanes, [](const NfcTapPartial &x, const NfcTapPartial &y) { return nfc_tap_partial_merge(x, y); });
      A.partials[j] = lanes[0];
   }
}

void nfc_tap_reduce_finish_kernel(NfcTapReduceArgs A)
{
   for (uint64_t t = 0; t < A.items * A.channels; t++)
      nfc_tap_reduce_finish(A, t);
}

/* ... and of the kernels of nfcgpu_apcm_encode (nfc_apcm.hip): the units and the entries of nfc_apcm.hpp as loops, a unit's points one
 * after the other where the device takes a tile of 64 at a time, the parts merged in sequence where it scans a wave. The staging
 * area and the way it is written out are the device's, lane by lane. */
void nfc_apcm_count_kernel(NfcApcmArgs A)
{
   for (uint64_t unit = 0; unit < A.units; unit++)
   {
      uint32_t buffer, begin, end, position;

      nfc_apcm_unit(A, unit, buffer, begin, end, position);

      const NfcApcmPair *row = nfc_apcm_row(A, buffer);
      NfcApcmPart run = nfc_apcm_none();

      for (uint32_t i = begin; i < end; i++)
      {
         const NfcApcmPoint p = nfc_apcm_point(A, row, position, i);

         if (p.keep)
            run = nfc_apcm_merge(run, nfc_apcm_single(p));
      }

      A.parts[unit] = run;
   }
}

void nfc_apcm_scan_kernel(NfcApcmArgs A)
{
   for (uint32_t entry = 0; entry < A.nEntries; entry++)
   {
      NfcApcmPart carry = nfc_apcm_start(A);

      for (uint64_t unit = (uint64_t)entry * A.unitsPerEntry; unit < ((uint64_t)entry + 1) * A.unitsPerEntry; unit++)
      {
         NfcApcmBase b;

         b.record = carry.kept;
         b.prevOffset = carry.last;
         b.prevSample = carry.sample;
         b.pad = 0;
         A.bases[unit] = b;
         carry = nfc_apcm_merge(carry, A.parts[unit]);
      }

      nfc_apcm_finish(A, entry, carry);
   }
}

void nfc_apcm_encode_kernel(NfcApcmArgs A)
{
   static uint32_t stage[NfcApcmShape::kStageDwords];

   for (uint64_t unit = 0; unit < A.units; unit++)
   {
      const uint32_t kept = A.parts[unit].kept;

      if (!kept)
         continue;

      const NfcApcmBase b = A.bases[unit];
      uint32_t buffer, begin, end, position, first, last, lead;

      nfc_apcm_unit(A, unit, buffer, begin, end, position);
      nfc_apcm_window(A, b.record, kept, first, last, lead);

      const NfcApcmPair *row = nfc_apcm_row(A, buffer);
      uint32_t beforeOffset = b.prevOffset, done = 0;
      int32_t beforeSample = b.prevSample;

      for (uint32_t i = begin; i < end && first + done < last; i++)
      {
         const NfcApcmPoint p = nfc_apcm_point(A, row, position, i);

         if (!p.keep)
            continue;

         nfc_apcm_stage(stage, lead, done++, nfc_apcm_record(p, beforeOffset, beforeSample));
         beforeOffset = p.offset;
         beforeSample = p.sample;
      }

      for (uint32_t lane = 0; lane < 64 && last > first; lane++)
         nfc_apcm_flush(nfc_apcm_window_at(A, buffer / A.buffersPerEntry, first, lead), stage, lead, 3u * (last - first), lane);
   }
}
#else
__global__ void nfc_apcm_count_kernel(NfcApcmArgs A);
__global__ void nfc_apcm_scan_kernel(NfcApcmArgs A);
__global__ void nfc_apcm_encode_kernel(NfcApcmArgs A);
__global__ void nfc_tap_reduce_kernel(NfcTapReduceArgs A);
__global__ void nfc_tap_reduce_finish_kernel(NfcTapReduceArgs A);
__global__ void nfc_tap_walk_kernel(NfcTapArgs A, NfcConfig cfg);
__global__ void nfc_tap_seam_kernel(NfcTapArgs A);
__global__ void nfc_tap_list_kernel(NfcTapArgs A);
__global__ void nfc_tap_finish_kernel(NfcTapArgs A);
#endif

/* ---- helper kernels of pipelined submissions (run_windowed): a thread per stream of the submission ----
 * The front of a submission (scan, seam rounds, planes) reads of a stream's slot the front-end state its first chunk starts from:
 * clock, pulse counter, envelope, filter, deviation, average, edge peak, edge time and the carrier zone (nfc_scan_begin, and the
 * edge time once more in nfc_seams_kernel). While the submission before is still in its tail the finish has not written those
 * yet - but the front end is a function of the samples: once that submission's seam rounds are over, the end of its last chunk
 * is the state its finish will write. nfc_shadow_kernel forms it; nfc_shadow_compare_kernel holds it against what the finish
 * really wrote, bit for bit on exactly those fields (the carrier times as the zone the front derives from them, which is all it
 * reads of them), and counts the streams that differ: exact or not taken.
 *
 * One difference is expected and is put right without a second walk. The decoder zeroes its copy of the edge time when it emits a
 * carrier frame (nfc_scan_begin's note), so a stream whose last carrier frame came after the tracker last moved ends with 0 where
 * its shadow holds the tracker's time T. Nothing a walk computes depends on the time it starts with: the tracker overwrites it with
 * clocks of the new submission's own samples, and until then the start value is only handed on - into the chunks' inherited times
 * (chunkEdge), into the start of a chunk that is walked again from its predecessor's end and from there into that walk's
 * records - and tested for equality against values of the same kind (nfc_seams_check, nfc_scan_adopt). T is a clock of an
 * earlier sample and 0 is not a clock of this submission either (the path keeps clear of the clock's wrap), so neither can
 * equal a time the tracker sets during the submission: every one of those tests falls the same way with 0 as with T, and the
 * records of the walk from 0 are the records at hand with T replaced by 0 wherever a record holds T as a known time.
 * nfc_shadow_rename_kernel does that for the streams the comparison found to differ in this way and in nothing else. */
struct NfcShadowArgs
{
   const NfcScanJob *jobs;
   uint32_t nJobs;
   const NfcScanSeam *seams;      /* shadow kernel: the records of the submission whose end is formed */
   const uint32_t *chunkEdge;
   const NfcStreamState *from;    /* shadow kernel: what that submission's front started from (the slots, or the shadows themselves) */
   NfcStreamState *shadow;        /* [maxStreams] */
   const NfcStreamState *real;    /* compare kernel: the slots */
   uint32_t *ctl;                 /* compare kernel: [0] streams that differ otherwise than by a zeroed edge time, [1..9] streams that differ in clock, pulse counter,
                                     envelope, n1, deviation, average, edge peak, edge time, carrier zone, [10] streams with a zeroed edge time alone;
                                     [16 + j]: stream j of the submission 0 same, 1 zeroed edge time alone, 2 differs */
   NfcScanPoint *points;          /* rename kernel: the records of the front that started from the shadows */
   NfcScanSeam *renameSeams;
   uint32_t *renameEdge;
   uint32_t spoil;                /* shadow kernel, test switch: 1 + the slot whose shadow is spoilt (0: none) */
};

#ifdef NFCGPU_EMULATED_TEST_BUILD
#define NFC_PIPE_FN static inline
#define NFC_PIPE_COUNT(p) (++*(p))
#else
#define NFC_PIPE_FN static __device__ __forceinline__
#define NFC_PIPE_COUNT(p) atomicAdd((p), 1u)
#endif

NFC_PIPE_FN uint32_t nfc_pipe_bits(float v)
{
   uint32_t u;
   __builtin_memcpy(&u, &v, 4);
   return u;
}

/* the carrier zone a walk starts in (nfc_scan_begin) */
NFC_PIPE_FN uint32_t nfc_pipe_zone(const NfcStreamState &s)
{
   return s.carrierOn ? 1u : (s.carrierOff ? 2u : 0u);
}

NFC_PIPE_FN void nfc_shadow_write(const NfcShadowArgs &S, uint32_t j)
{
   const NfcScanJob &job = S.jobs[j];

   if (job.chunks == 0u)
      return;

   const uint32_t last = job.firstChunk + job.chunks - 1u;
   const NfcScanPoint &end = S.seams[last].end;

   NfcStreamState s = S.from[job.slot];

   s.clock += job.count;
   s.pulseFilter = end.pulseFilter;
   s.env = end.env;
   s.n1 = end.n1;
   s.mdev = end.mdev;
   s.avg = end.avg;
   s.edgePeak = end.edgePeak;
   /* the edge tracker's time: the walk's own where it has set one (NFC_ZONE_EDGE_KNOWN of nfc_scan.hpp), else the one the last chunk
    * inherited. The decoder's copy is zeroed by a carrier frame (nfc_scan_begin's note): a stream that emitted one after the
    * tracker last moved differs here, is found by the comparison and has the time put right in its records (nfc_shadow_rename). */
   s.edgeTime = (end.zone & 0x100u) ? end.edgeTime : S.chunkEdge[last];
   s.carrierOn = (end.zone & 0xFFu) == 1u ? 1u : 0u;
   s.carrierOff = (end.zone & 0xFFu) == 2u ? 1u : 0u;

   if (S.spoil == job.slot + 1u)
      s.avg = -s.avg - 1.0f;

   S.shadow[job.slot] = s;
}

NFC_PIPE_FN void nfc_shadow_compare(const NfcShadowArgs &S, uint32_t j)
{
   const NfcStreamState &a = S.real[S.jobs[j].slot], &b = S.shadow[S.jobs[j].slot];

   const bool differ[9] = {a.clock != b.clock,
                           a.pulseFilter != b.pulseFilter,
                           nfc_pipe_bits(a.env) != nfc_pipe_bits(b.env),
                           nfc_pipe_bits(a.n1) != nfc_pipe_bits(b.n1),
                           nfc_pipe_bits(a.mdev) != nfc_pipe_bits(b.mdev),
                           nfc_pipe_bits(a.avg) != nfc_pipe_bits(b.avg),
                           nfc_pipe_bits(a.edgePeak) != nfc_pipe_bits(b.edgePeak),
                           a.edgeTime != b.edgeTime,
                           nfc_pipe_zone(a) != nfc_pipe_zone(b)};
   bool any = false;

   for (int i = 0; i < 9; i++)
   {
      if (differ[i])
         NFC_PIPE_COUNT(S.ctl + 1 + i);
      any = any || differ[i];
   }

   const bool zeroed = differ[7] && !(differ[0] || differ[1] || differ[2] || differ[3] || differ[4] || differ[5] || differ[6] || differ[8]) && a.edgeTime == 0u;

   if (any)
      NFC_PIPE_COUNT(zeroed ? S.ctl + 10 : S.ctl);

   S.ctl[16 + j] = any ? (zeroed ? 1u : 2u) : 0u;
}

/* thread `lane` of `lanes` for stream j: the shadow's edge time becomes 0 wherever a record of the stream's front holds it as a known time */
NFC_PIPE_FN void nfc_shadow_rename(const NfcShadowArgs &S, uint32_t j, uint32_t lane, uint32_t lanes)
{
   if (S.ctl[16 + j] != 1u)
      return;

   const NfcScanJob &job = S.jobs[j];
   const uint32_t was = S.shadow[job.slot].edgeTime;

   for (uint32_t k = lane; k < job.chunks; k += lanes)
   {
      NfcScanSeam &s = S.renameSeams[job.firstChunk + k];
      if ((s.start.zone & 0x100u) && s.start.edgeTime == was)
         s.start.edgeTime = 0u;
      if ((s.end.zone & 0x100u) && s.end.edgeTime == was)
         s.end.edgeTime = 0u;
      if (S.renameEdge[job.firstChunk + k] == was)
         S.renameEdge[job.firstChunk + k] = 0u;
   }

   const uint32_t nPoints = job.count / NFC_SCAN_POINT + 1u;

   for (uint32_t i = lane; i < nPoints; i += lanes)
   {
      NfcScanPoint &p = S.points[job.firstPoint + i];
      if ((p.zone & 0x100u) && p.edgeTime == was)
         p.edgeTime = 0u;
   }
}

#ifdef NFCGPU_EMULATED_TEST_BUILD
void nfc_shadow_kernel(NfcShadowArgs S)
{
   for (uint32_t j = 0; j < S.nJobs; j++)
      nfc_shadow_write(S, j);
}

void nfc_shadow_compare_kernel(NfcShadowArgs S)
{
   for (uint32_t j = 0; j < S.nJobs; j++)
      nfc_shadow_compare(S, j);
}

void nfc_shadow_rename_kernel(NfcShadowArgs S)
{
   for (uint32_t j = 0; j < S.nJobs; j++)
      nfc_shadow_rename(S, j, 0u, 1u);
}
#else
__global__ void nfc_shadow_kernel(NfcShadowArgs S)
{
   const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
   if (j < S.nJobs)
      nfc_shadow_write(S, j);
}

__global__ void nfc_shadow_compare_kernel(NfcShadowArgs S)
{
   const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
   if (j < S.nJobs)
      nfc_shadow_compare(S, j);
}

/* (a workgroup per stream) */
__global__ void nfc_shadow_rename_kernel(NfcShadowArgs S)
{
   if (blockIdx.x < S.nJobs)
      nfc_shadow_rename(S, blockIdx.x, threadIdx.x, blockDim.x);
}
#endif

namespace {

constexpr uint32_t kMaxConfigs = 256; /* distinct decoder configurations in use at once (1.5 KB each on the device) */
constexpr uint32_t kRingBlockFloats = (4 * NFC_HIST_STORED + NFC_PROD + NFC_CORR_MAX) * NFC_LANES;

struct StreamInfo
{
   bool open = false;
   bool initialized = false; /* device state valid */
   bool needInit = true;
   bool explicitInit = false; /* the pending initialisation was asked for (initialize()), not caused by a buffer */
   bool listed = false; /* part of the batch being submitted */
   nfcgpu_params params {};
   float powerAtInit = 0.01f; /* carrier thresholds are derived when the decoder (re)initialises */
   uint32_t config = 0;
   bool hasConfig = false; /* `config` has been resolved (a stream opened but never fed refers to no table entry) */
   uint32_t derivedRate = 0; /* sample rate the running configuration was derived from (params.sample_rate is the stored one) */
   uint32_t clock = 0xFFFFFFFFu; /* mirror of the device sample clock (NfcStreamState::clock) */
   std::deque<nfcgpu_frame> queue;
};

/* true when a stream whose clock mirror reads `clock` is, during a submission of `count` samples, within 1024 samples
 * of its start or of the 32-bit clock wrap (same test as nfc_exact_span in nfc_kernels.hip, which decides per stream
 * block). The mirror itself is only advanced once the launch has been issued (commit_clock). */
bool exact_zone(uint32_t clock, uint32_t count)
{
   const uint32_t start = clock + 1u + 1024u;
   const uint32_t untilWrap = 0u - start;
   return count != 0 && (start < 2048u || untilWrap < count);
}

void commit_clock(StreamInfo &si, uint32_t count)
{
   si.clock += count;
}

struct ProfiledLaunch
{
   hipEvent_t start;
   hipEvent_t stop;
};

struct WindowedTail;

}

struct nfcgpu_ctx
{
   int device = 0;
   hipStream_t stream = nullptr;
   hipStream_t side = nullptr;       /* the carry lanes of a windowed pass run beside the speculative ones */
   uint32_t sideMode = 2;            /* NFCGPU_SIDE_STREAM: 0 one stream, 1 two fixed events, 2 events per pass */
   hipEvent_t forkEvent = nullptr, joinEvent = nullptr;
   hipStream_t low = nullptr;        /* lowest priority: the walk that writes the planes beside the rounds of second walks */
   uint32_t maxStreams = 0;
   uint32_t blocks = 0;

   NfcStreamState *dStates = nullptr;
   NfcStreamCold *dCold = nullptr;
   float *dRings = nullptr;
   uint8_t *dBytes = nullptr;
   uint32_t *dSink = nullptr;
   uint32_t *dSinkCtl = nullptr;
   uint64_t sinkWords = 0;
   uint32_t *ownSink = nullptr; /* the context's own sink, kept while a caller-provided one is attached */
   uint32_t *ownSinkCtl = nullptr;
   uint64_t ownSinkWords = 0;
   NfcWork *dWorks = nullptr;
   NfcConfig *dConfigs = nullptr;
   bool genericOnly = false; /* NFCGPU_GENERIC_KERNELS=1: never use the sample-rate-specialised kernels (testing) */
   /* Staging of host-resident input: two slots, each a device buffer with a pinned mirror. Caller memory is copied into
    * the mirror by the CPU and never handed to the GPU runtime (no page locking of memory whose lifetime belongs to the
    * caller); the copy to the device and the launches that read it are asynchronous, and an event recorded behind them
    * says when the slot may be written again. A submission therefore does not wait for its own kernels. */
   struct StageSlot
   {
      uint8_t *d = nullptr;
      uint8_t *h = nullptr;
      size_t bytes = 0;
      hipEvent_t done = nullptr;
      bool busy = false;
   };
   StageSlot stage[2];
   uint32_t stageNext = 0;
   bool inflight = false; /* something has been enqueued since the last stream synchronisation */
#ifdef NFCGPU_EMULATED_TEST_BUILD
   std::vector<std::vector<float>> widened; /* TEST SCAFFOLDING: int16 input widened for the twins (widen_i16), kept until the next sync */
#endif

   std::vector<NfcConfig> configs;
   std::vector<StreamInfo> streams;
   std::vector<NfcWork> hWorks;
   std::vector<uint32_t> hSink;

   bool hold = false;
   bool profile = false;
   bool dirty = false; /* work submitted since last sync */
   uint32_t launchSeq = 0; /* stamp of the last demodulation launch (NfcLaunch::launchSeq) */

   /* ---- time-parallel path (nfc_scan.h): device buffers, grown on demand and kept ---- */
   bool windowed = true;           /* NFCGPU_WINDOWED=0 switches the path off */
   uint32_t windowedMinSamples = 32768; /* shortest submission (per stream) worth cutting into windows */
   uint32_t scanChunk = 8192;      /* samples per scan chunk, at least: short chunks = many lanes (the walk is latency-bound per wave) */
   uint32_t scanLanes = 32768;     /* chunks a large submission is cut into, at least (NFCGPU_SCAN_LANES) */
   bool scanChunkFixed = false;    /* NFCGPU_SCAN_CHUNK given: no sizing by the submission */
   uint32_t blockSamples = 1u << 23; /* a few long busy streams are decoded this many samples at a time (NFCGPU_BLOCK_SAMPLES) */
   bool inBlocks = false;
   uint32_t scanWarm = 4096;       /* samples walked ahead of a chunk (round 4: 6144 -> 4096; config 5 dense: scan and second walks 94 -> 79 ms per step, as many chunks walked again) */
   uint32_t maxPasses = 32;        /* decode passes before a stream of a large submission gives up (sequential path). Round 4: 12 -> 32: a late pass of a
                                      few lanes is 10-20 ms, the sequential kernels take seconds for a stream of 2^20 samples (256 dense streams x 2^20
                                      cut into 64 lanes each: one stream in 768 needed a thirteenth pass, and the step took 1035 instead of 305 ms) */
   uint32_t maxPassesFew = 48;     /* the same for submissions of fewer streams than a wave has lanes: the sequential path would crawl */
   struct DevBuf
   {
      void *ptr = nullptr;
      size_t bytes = 0;
   };
   DevBuf wRepairs, wJobs, wChunks, wPoints, wSeams, wChunkEdge, wTiles, wTileStats, wWindows, wWorks, wCounters, wRunList;
   uint32_t busyPercent = 8;   /* a stream with more than this share of busy tiles is "busy": few long busy streams are decoded in blocks */
   DevBuf vStates, vCold, vRings, vBytes, vSink, vSinkCtl, vSaveRings, vSaveBytes;
   uint32_t longFirst = 32768;      /* the run list of a pass takes its lanes longest first, by classes of their length down to this one (NFCGPU_LONG_FIRST; 0: as they come) */
   uint32_t lanesWanted = 4096;     /* lanes a large busy submission is cut into, at least (NFCGPU_LANES_WANTED; 0: always NFC_WINDOW_CUT apart). Round 4: 16384 -> 4096: longer lanes need fewer passes (512 dense streams x 2^20: 320 -> 273 ms per step; 4096 streams are at NFCGPU_CUT_MAX either way) */
   uint32_t cutMax = 1u << 19;      /* ... but never further apart than this (NFCGPU_CUT_MAX). Round 5: 2^19 instead of 2^17 - config 5 at 2^17, 2^18,
                                       2^19, 2^20: 458, 456, 452, 452 ms per step (three runs each at 2^17 and 2^19: +-1 ms); 2^16: 500, 2^15: 555. Most
                                       lanes begin after quiet signal, not at a cut; the fewer cuts, the fewer guesses */
   uint32_t stagingWords = 0;       /* NFCGPU_STAGING_WORDS: cap on the lanes' staging sink (0: none) */
   uint32_t soloSamples = 1u << 15; /* streams this short are decoded by their carry lane alone, in one pass (NFCGPU_SOLO_SAMPLES). Round 4: 2^18 -> 2^16,
                                       the lanes being what they now are: the bundled captures of 100 k - 200 k samples 25 / 39 / 49 -> 17 / 27 / 37 ms.
                                       Round 6: 2^16 -> 2^15. A 65536-sample buffer is what the reference's task hands the decoder per call
                                       (TS/main.cpp:163-165, RadioDecoderTask.cpp:377-401), and a lane without windows can retire to nobody: it walked
                                       all 1024 tiles of a buffer with nothing in it (7 ms). The task on the shim in its default mode, dense / sparse
                                       WAV: 4.9 / 6.4 -> 8.3 / 15.1 MS/s (profiles/r06/shim_default_mode.txt) */
   DevBuf wPlanes, wPlaneChunks;   /* front-end planes (NfcScanArgs::planes) and the chunk list of the walk that writes them */
   DevBuf wRepairsEnv;             /* the chunks of a round whose envelope tracker alone is walked again (nfc_envelope_kernel) */
   uint32_t envelopeMax = 16384;   /* ... when the round lists at most this many of them (NFCGPU_ENVELOPE_KERNEL; 0: never, one list for the scan kernel).
                                      Round 5: a wavefront per chunk (nfc_envelope.hpp). Round 4's kernel had a lane per chunk - good for the few
                                      4096-sample chunks of a short capture's rounds, the wrong shape for the long lists of a large submission
                                      (thousands of lanes reading 32768-sample chunks a cache line each: 79 -> 122 ms per step of the headline,
                                      profiles/r04/ab_envelope) - and was given lists of at most 64 */
   DevBuf wPlanesStale;            /* NfcScanArgs::planesStale */

   /* ---- pipelined submissions (run_windowed): the front of a submission under the tail of the one before ---- */
   bool pipeline = true;           /* NFCGPU_PIPELINE=0: every submission is complete when its call returns */
   WindowedTail *tail = nullptr; /* the pending tail: every entry point completes it first (settle_tail) */
   hipStream_t front = nullptr;    /* the stream of a front that runs under a tail (the planes stay on `low`) */
   hipEvent_t frontEvent = nullptr, planesFork = nullptr, planesJoin = nullptr;
   DevBuf otherSet[13];            /* the second set of the buffers a front writes and a tail still reads (swap_front_sets), allocated when a
                                      submission first finds a tail pending: about as much again as the first, nearly all of it planes */
   DevBuf wShadow, wShadowCtl;     /* NfcShadowArgs::shadow, ::ctl */
   bool noSecondSet = false;       /* the device could not give the second set: no overlap for this context */
   bool growingSecond = false;
   bool deferOK = false;           /* the submission at hand may leave its tail pending (nfcgpu_submit_uniform) */
   bool dumpWindows = false;       /* NFCGPU_DUMP_WINDOWS is set (tuning build) */
   bool pipelineReport = false;    /* NFCGPU_PIPELINE_REPORT is set (tuning build): a line on stderr per comparison of shadows and slots */
   uint32_t spoilShadow = 0;       /* test switch of the tuning / emulated builds (NFCGPU_TEST_SPOIL_SHADOW): NfcShadowArgs::spoil */
   uint32_t *tailHost = nullptr;   /* pinned words of the read-backs: [0] chain "again", [1] run list length, [2..3] staging sink control, [16..31] shadow comparison */
   uint32_t *frontHost = nullptr;  /* ... of the front: [0..2] repair counts of a round, [4] stale plane chunks */
   NfcScanJob *tailJobs = nullptr; /* pinned: the job table as the finish left it */
   size_t tailJobsBytes = 0;
   uint32_t planesBeside = 1;      /* the walk that writes a large submission's planes runs on the side stream beside the rounds of second walks that follow the
                                      first (NFCGPU_PLANES_BESIDE; 0: after them, as until round 5) */
   uint32_t planesBesidePiece = 2048; /* ... samples per lane of that walk, from the stored points (NFCGPU_PLANES_BESIDE_PIECE; 0: a lane per chunk, from its start).
                                      Config 5, ms per step: after the rounds 452.7; beside them a lane per chunk 442.8, per 8192 / 2048 / 512 samples 438.5 / 436.7 / 437.6 */
   uint32_t planesPiece = 512;     /* samples per lane of the walk that writes a small submission's front-end planes (NFCGPU_PLANES_PIECE; 0: a lane per chunk) */
   uint32_t envelopeFollowMax = 1024; /* ... and a walk goes on through the chain of chunks that inherit its chunk's envelope when the round lists at
                                         most this many (NFCGPU_ENVELOPE_FOLLOW): the tail of rounds with a few chunks each becomes one or two rounds
                                         (a short capture: ten rounds -> three, 3.9 -> 2.6 ms; config 5: seven -> five). Not for the long lists: a
                                         chain is then one wavefront's serial work while the rest of the device waits (seams 40 -> 46 ms with it) */
   std::vector<ProfiledLaunch> timedScan, timedWindow, timedWave, timedPlanes;
   hipEvent_t epoch = nullptr;      /* recorded when the statistics start over: the time base of the launch intervals below */
   std::vector<std::pair<float, float>> waveSpans; /* [start, stop) of every wave decoder launch since, ms after `epoch` */
   double waveBusyMs = 0.0;         /* ... and the union of those that have been folded away (fold_wave_spans) */

   /* ---- frame gather over RCCL (nfcgpu_comm_*) ---- */
   void *comm = nullptr;
   int commRank = 0, commRanks = 0;
   uint32_t *dCounts = nullptr;
   std::vector<ProfiledLaunch> timed;
   std::vector<hipEvent_t> eventPool;
   nfcgpu_stats stats {};
   std::string lastError;

   /* nfcgpu_spectrum: window and twiddle tables on the device, one block per (length, window) used so far, kept */
   struct SpectrumTables
   {
      uint32_t length = 0, window = 0;
      float *d = nullptr; /* `length` window factors, then `length` twiddles (float2) */
   };
   std::vector<SpectrumTables> spectrumTables;

   /* nfcgpu_record: one partial per segment of every buffer of a call (device), grown on demand, kept */
   void *recordPartials = nullptr;
   size_t recordPartialsBytes = 0;
   /* nfcgpu_signal_tap: the walkers' start and end states, the frontiers and the list of a call (device), grown on demand, kept;
    * the length of a round's list as the host reads it (pinned) */
   void *tapScratch = nullptr;
   size_t tapScratchBytes = 0;
   uint32_t *tapCount = nullptr;
   /* nfcgpu_signal_tap_reduce: the planes of a slab, the partials of its units and the flag word (device), grown on demand, kept */
   void *tapReduceScratch = nullptr;
   size_t tapReduceScratchBytes = 0;

   /* nfcgpu_apcm_encode: the parts and the bases of the units and the flag word (device), grown on demand, kept */
   void *apcmScratch = nullptr;
   size_t apcmScratchBytes = 0;
};

namespace {

int fail(nfcgpu_ctx *ctx, int code, const char *what, hipError_t err = hipSuccess)
{
   if (ctx)
   {
      ctx->lastError = what;
      if (err != hipSuccess)
      {
         ctx->lastError += ": ";
         ctx->lastError += hipGetErrorString(err);
      }
   }
   return code;
}

#define HIP_TRY(ctx, call)                                   \
   do                                                        \
   {                                                         \
      hipError_t err__ = (call);                             \
      if (err__ != hipSuccess)                               \
         return fail((ctx), NFCGPU_EHIP, #call, err__);      \
   } while (0)

NfcLaunch base_launch(nfcgpu_ctx *ctx)
{
   NfcLaunch L;
   std::memset(&L, 0, sizeof(L));
   L.states = ctx->dStates;
   L.cold = ctx->dCold;
   L.rings = ctx->dRings;
   L.bytes = ctx->dBytes;
   L.sink = ctx->dSink;
   L.sinkCtl = ctx->dSinkCtl;
   L.sinkWords = (uint32_t)ctx->sinkWords;
   L.ringBlockFloats = kRingBlockFloats;
   return L;
}

/* true when every sample-rate-derived constant of `cfg` equals the table compiled into the specialised kernels
 * (thresholds and the enable mask are run-time values there as well) */
bool matches_fixed_table(const NfcConfig &cfg)
{
   if (cfg.sampleRate != NFC_FIXED_SAMPLE_RATE)
      return false;

   NfcConfig probe = cfg;
   nfc_fixed_config(probe);
   return std::memcmp(&probe, &cfg, sizeof(cfg)) == 0;
}

/* find or create the device-side NfcConfig for a stream's parameters */
int resolve_config(nfcgpu_ctx *ctx, StreamInfo &si)
{
   NfcHostParams hp;
   hp.sampleRate = si.derivedRate;
   hp.enabled = si.params.tech_mask & 0xF;
   hp.powerLevelThreshold = si.params.power_level_threshold;
   for (int t = 0; t < 4; t++)
   {
      hp.corrThreshold[t] = si.params.corr_threshold[t];
      hp.minDepth[t] = si.params.min_modulation_depth[t];
      hp.maxDepth[t] = si.params.max_modulation_depth[t];
   }

   NfcConfig cfg;
   if (!nfc_build_config(hp, cfg))
      return fail(ctx, NFCGPU_ERATE, "sample rate not decodable with the fixed history depth");

   /* signalLow/HighThreshold are only recomputed by initialize() (NfcDecoder.cpp:327-329) */
   cfg.lowThreshold = si.powerAtInit / 1.25f;
   cfg.highThreshold = si.powerAtInit * 1.25f;

   for (uint32_t i = 0; i < ctx->configs.size(); i++)
   {
      if (std::memcmp(&ctx->configs[i], &cfg, sizeof(cfg)) == 0)
      {
         si.config = i;
         si.hasConfig = true;
         return NFCGPU_OK;
      }
   }

   if (ctx->configs.size() < kMaxConfigs)
   {
      ctx->configs.push_back(cfg);
      si.config = (uint32_t)ctx->configs.size() - 1;
   }
   else
   {
      /* the table is full: take the place of a configuration no open stream refers to any more (parameters changed
       * since, streams closed). Launches that may still read it are waited for first. */
      std::vector<bool> used(kMaxConfigs, false);
      for (const StreamInfo &other: ctx->streams)
      {
         if (other.open && &other != &si && other.hasConfig)
            used[other.config] = true;
      }

      uint32_t slot = kMaxConfigs;
      for (uint32_t i = 0; i < kMaxConfigs && slot == kMaxConfigs; i++)
      {
         if (!used[i])
            slot = i;
      }

      if (slot == kMaxConfigs)
         return fail(ctx, NFCGPU_ENOMEM, "too many distinct decoder configurations in use at once");

      HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
      ctx->configs[slot] = cfg;
      si.config = slot;
   }

   si.hasConfig = true;

   HIP_TRY(ctx, hipMemcpyAsync(ctx->dConfigs + si.config, &cfg, sizeof(cfg), hipMemcpyHostToDevice, ctx->stream));
   HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); /* cfg is a stack object */

   return NFCGPU_OK;
}

/* The reference keeps two things apart: the sample rate it stores (setSampleRate(), or taken from a buffer whose rate
 * differs from the stored one, NfcDecoder.cpp:383-388) and the parameters initialize() derived from the rate stored at
 * that moment (NfcDecoder.cpp:295-360). A buffer only re-initialises the decoder when its rate differs from the stored
 * one, so after setSampleRate(x) buffers labelled x are decoded with the parameters of the previous rate. The one thing
 * not reproduced: parameters derived while the stored rate was still 0 (initialize() before any rate is known, then the
 * rate given through the setter) leave the reference with NaN filter weights and no output; here they are derived when
 * the first buffer arrives. */
int adopt_sample_rate(nfcgpu_ctx *ctx, StreamInfo &si, uint32_t sampleRate)
{
   if (sampleRate == 0)
      return fail(ctx, NFCGPU_EINVAL, "sample rate must be non-zero");

   if (si.params.sample_rate != sampleRate)
   {
      /* frames are stamped with the rate stored when they were produced (NfcDecoder.cpp frame.setSampleRate): collect
       * what the sink holds before the stored rate changes */
      if (si.params.sample_rate != 0 && ctx->dirty && !ctx->hold)
      {
         int rc = nfcgpu_sync(ctx);
         if (rc != NFCGPU_OK && rc != NFCGPU_EOVERFLOW)
            return rc;
      }

      si.params.sample_rate = sampleRate;
      si.derivedRate = sampleRate;
      si.needInit = true;
      si.explicitInit = false; /* the reference initialises again, with what is set now */
   }
   else if (!si.initialized || si.derivedRate == 0)
   {
      si.needInit = true;
   }

   if (si.needInit)
   {
      if (si.derivedRate == 0)
         si.derivedRate = sampleRate;

      /* the carrier thresholds follow the power level of the moment of the initialisation (NfcDecoder.cpp:327-329):
       * the moment of initialize() if that is what is pending, now otherwise */
      if (!si.explicitInit)
         si.powerAtInit = si.params.power_level_threshold;

      si.explicitInit = false;
      return resolve_config(ctx, si);
   }

   return NFCGPU_OK;
}

/* run nfc_init_kernel for every stream in [first, first+count) that needs it (listedOnly: and is part of the batch
 * being submitted; a stream opened but not yet fed has no configuration resolved); contiguous runs with equal
 * (config, keep) share one launch */
int initialize_pending(nfcgpu_ctx *ctx, uint32_t first, uint32_t count, bool listedOnly)
{
   uint32_t i = first;
   const uint32_t end = first + count;

   auto due = [&](const StreamInfo &si) { return si.open && si.needInit && (si.listed || !listedOnly); };

   while (i < end)
   {
      StreamInfo &si = ctx->streams[i];

      if (!due(si))
      {
         i++;
         continue;
      }

      const uint32_t cfg = si.config;
      const bool keep = si.initialized;
      uint32_t j = i;

      while (j < end && due(ctx->streams[j]) && ctx->streams[j].config == cfg && ctx->streams[j].initialized == keep)
         j++;

      NfcLaunch L = base_launch(ctx);
      L.firstSlot = i;
      L.slotCount = j - i;

      const uint32_t threads = 64;
      const uint32_t grid = (L.slotCount + threads - 1) / threads;

      hipLaunchKernelGGL(nfc_init_kernel, dim3(grid), dim3(threads), 0, ctx->stream, ctx->dConfigs + cfg, L, keep ? 1u : 0u);
      HIP_TRY(ctx, hipGetLastError());

      for (uint32_t k = i; k < j; k++)
      {
         ctx->streams[k].needInit = false;
         ctx->streams[k].initialized = true;
         ctx->streams[k].clock = 0xFFFFFFFFu;
      }

      i = j;
   }

   return NFCGPU_OK;
}

hipEvent_t take_event(nfcgpu_ctx *ctx)
{
   if (!ctx->eventPool.empty())
   {
      hipEvent_t e = ctx->eventPool.back();
      ctx->eventPool.pop_back();
      return e;
   }
   hipEvent_t e = nullptr;
   (void)hipEventCreate(&e);
   return e;
}

int launch_demod(nfcgpu_ctx *ctx, uint32_t config, NfcLaunch &L, uint64_t samples, bool exactPossible, bool exactOnly)
{
   const uint32_t firstBlock = L.firstSlot / NFC_LANES;
   const uint32_t lastBlock = (L.firstSlot + L.slotCount - 1) / NFC_LANES;

   L.firstBlock = firstBlock;

   ProfiledLaunch pl {nullptr, nullptr};

   if (ctx->profile)
   {
      pl.start = take_event(ctx);
      pl.stop = take_event(ctx);
      HIP_TRY(ctx, hipEventRecord(pl.start, ctx->stream));
   }

   const bool fixed = !ctx->genericOnly && matches_fixed_table(ctx->configs[config]);

   /* every stream block picks its kernel from the device state; a launch in which every stream needs the exact
    * variant (the first buffer of freshly opened streams) does not need the common kernel at all */
   L.forceExact = exactOnly ? 1u : 0u;

   if (++ctx->launchSeq == 0)
      ctx->launchSeq = 1;
   L.launchSeq = ctx->launchSeq;

   if (!exactOnly)
   {
      hipLaunchKernelGGL(fixed ? NFC_BY_LAYOUT(L.uniformStride, nfc_demod_fixed_kernel) : NFC_BY_LAYOUT(L.uniformStride, nfc_demod_kernel), dim3(lastBlock - firstBlock + 1), dim3(NFC_LANES), 0,
                         ctx->stream, ctx->dConfigs + config, L);
      HIP_TRY(ctx, hipGetLastError());
   }

   /* stream blocks near their start / the clock wrap skip the kernel above and are handled by this one */
   if (exactPossible)
   {
      hipLaunchKernelGGL(fixed ? NFC_BY_LAYOUT(L.uniformStride, nfc_demod_fixed_exact_kernel) : NFC_BY_LAYOUT(L.uniformStride, nfc_demod_exact_kernel), dim3(lastBlock - firstBlock + 1),
                         dim3(NFC_LANES), 0, ctx->stream, ctx->dConfigs + config, L);
      HIP_TRY(ctx, hipGetLastError());
   }

   if (ctx->profile)
   {
      HIP_TRY(ctx, hipEventRecord(pl.stop, ctx->stream));
      ctx->timed.push_back(pl);
   }

   ctx->stats.launches++;
   ctx->stats.samples += samples;
   ctx->dirty = true;

   return NFCGPU_OK;
}

/* ------------------------------------------------------------------------------------------ */
/* time-parallel path (nfc_scan.h)                                                             */
/* ------------------------------------------------------------------------------------------ */

struct WindowedItem
{
   uint32_t slot;
   const uint8_t *data; /* device */
   uint32_t count;
};

int grow(nfcgpu_ctx *ctx, nfcgpu_ctx::DevBuf &b, size_t bytes)
{
   if (bytes <= b.bytes)
      return NFCGPU_OK;

#ifdef NFCGPU_EMULATED_TEST_BUILD
   /* (test build: a device that cannot give the front-end planes more than this - the fallbacks of run_windowed) */
   if (const char *limit = std::getenv("NFCGPU_TEST_ALLOC_LIMIT"))
   {
      if (&b == &ctx->wPlanes && bytes > std::strtoull(limit, nullptr, 10))
         return fail(ctx, NFCGPU_ENOMEM, "device allocation for the time-parallel path failed (test limit)");
   }
   if (const char *limit = std::getenv("NFCGPU_TEST_ALLOC_LIMIT_SECOND"))
   {
      /* (... more than this for the planes of the second buffer set of pipelined submissions) */
      if (ctx->growingSecond && &b == &ctx->wPlanes && bytes > std::strtoull(limit, nullptr, 10))
         return fail(ctx, NFCGPU_ENOMEM, "device allocation for the time-parallel path failed (test limit)");
   }
   if (const char *limit = std::getenv("NFCGPU_TEST_ALLOC_LIMIT_LANES"))
   {
      /* (the same for a buffer that is grown elsewhere in run_windowed: the lanes' decoder states) */
      if (&b == &ctx->vStates && bytes > std::strtoull(limit, nullptr, 10))
         return fail(ctx, NFCGPU_ENOMEM, "device allocation for the time-parallel path failed (test limit)");
   }
#endif

   if (b.ptr)
   {
      HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
      (void)hipFree(b.ptr);
   }

   b.ptr = nullptr;
   b.bytes = 0;

   /* some room to grow into (a quarter; little for the buffers that are gigabytes), none when that does not fit */
   size_t want = bytes + (bytes < ((size_t)1 << 30) ? bytes / 4 : bytes / 32) + 256;

   if (hipMalloc(&b.ptr, want) != hipSuccess)
   {
      (void)hipGetLastError();
      want = bytes;

      if (hipMalloc(&b.ptr, want) != hipSuccess)
      {
         size_t freeBytes = 0, totalBytes = 0;
         (void)hipGetLastError();
         (void)hipMemGetInfo(&freeBytes, &totalBytes);
         b.ptr = nullptr;
         char what[160];
         std::snprintf(what, sizeof(what), "device allocation for the time-parallel path failed (%.2f GiB wanted, %.2f of %.2f GiB free)", (double)bytes / (double)(1 << 30),
                       (double)freeBytes / (double)(1 << 30), (double)totalBytes / (double)(1 << 30));
         return fail(ctx, NFCGPU_ENOMEM, what);
      }
   }

   b.bytes = want;
   return NFCGPU_OK;
}

/* the sequential kernels over a subset of slots (fallback of the time-parallel path). `stride` here and in everything below
 * that takes one is the submission's sample layout (nfc_sample.hpp): the components per sample, 1 or 2, for floats - the value it
 * has always been -, with NFC_SAMPLE_I16 set for int16 input */
int launch_sequential(nfcgpu_ctx *ctx, uint32_t config, const std::vector<WindowedItem> &items, uint32_t stride)
{
   if (items.empty())
      return NFCGPU_OK;

   /* a long first buffer of fresh streams: only its first samples need the exact-modulo kernel (which is chosen per
    * launch and is the slower one), so they get a launch of their own */
   {
      const uint32_t head = 2048;
      bool split = false;
      for (const WindowedItem &it: items)
         split = split || (ctx->streams[it.slot].clock == 0xFFFFFFFFu && it.count > 2 * head);

      if (split)
      {
         std::vector<WindowedItem> first, rest;
         for (const WindowedItem &it: items)
         {
            const uint32_t n = it.count < head ? it.count : head;
            first.push_back(WindowedItem {it.slot, it.data, n});
            if (it.count > n)
               rest.push_back(WindowedItem {it.slot, it.data + (size_t)n * nfc_sample_bytes(stride), it.count - n});
         }

         int rc = launch_sequential(ctx, config, first, stride);
         if (rc)
            return rc;
         return launch_sequential(ctx, config, rest, stride);
      }
   }

   uint32_t first = 0xFFFFFFFFu, last = 0;
   uint64_t samples = 0;
   bool exactPossible = false, exactOnly = true;

   for (const WindowedItem &it: items)
   {
      first = it.slot < first ? it.slot : first;
      last = it.slot > last ? it.slot : last;
   }

   std::vector<NfcWork> table(last - first + 1);
   for (NfcWork &w: table)
   {
      w.data = nullptr;
      w.count = 0;
      w.stride = 1;
      w.tiles = nullptr;
   }

   for (const WindowedItem &it: items)
   {
      NfcWork &w = table[it.slot - first];
      w.data = it.data;
      w.count = it.count;
      w.stride = stride;
      samples += it.count;
      const bool exact = exact_zone(ctx->streams[it.slot].clock, it.count);
      exactPossible = exactPossible || exact;
      exactOnly = exactOnly && (exact || it.count == 0);
   }

   HIP_TRY(ctx, hipMemcpyAsync(ctx->dWorks + first, table.data(), sizeof(NfcWork) * table.size(), hipMemcpyHostToDevice, ctx->stream));
   HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); /* `table` is a local */

   NfcLaunch L = base_launch(ctx);
   L.works = ctx->dWorks;
   L.uniformStride = stride;
   L.firstSlot = first;
   L.slotCount = last - first + 1;

   int rc = launch_demod(ctx, config, L, samples, exactPossible, exactOnly);
   if (rc)
      return rc;

   for (const WindowedItem &it: items)
      commit_clock(ctx->streams[it.slot], it.count);

   return NFCGPU_OK;
}

uint32_t tail_ahead(const nfcgpu_ctx *ctx, uint32_t slot);
int settle_tail(nfcgpu_ctx *ctx);
void stage_release(nfcgpu_ctx *ctx, nfcgpu_ctx::StageSlot *slot);

/* may these streams take the time-parallel path for this submission? (one configuration, one sample format) */
bool windowed_eligible(nfcgpu_ctx *ctx, uint32_t config, const std::vector<WindowedItem> &items)
{
   if (!ctx->windowed || ctx->genericOnly || items.empty() || !matches_fixed_table(ctx->configs[config]))
      return false;

   for (const WindowedItem &it: items)
   {
      if (it.count < ctx->windowedMinSamples)
         return false;

      /* stay clear of the 32-bit wrap of the sample clock: the lanes number their rings from their own first sample
       * and never take the exact-modulo route (a fresh stream, clock 0xFFFFFFFF, is handled by its carry lane) */
      uint32_t clock = ctx->streams[it.slot].clock;
      if (const uint32_t ahead = tail_ahead(ctx, it.slot))
         clock += ahead; /* (the mirror follows when the pending tail completes: the clock that submission will leave) */
      if (clock != 0xFFFFFFFFu && (uint64_t)clock + it.count + 4096u >= 0xFFFFFFFFull)
         return false;
   }

   return true;
}

void record_span(nfcgpu_ctx *ctx, std::vector<ProfiledLaunch> &into, ProfiledLaunch &pl, bool begin, hipStream_t on = nullptr)
{
   if (!ctx->profile)
      return;

   if (!on)
      on = ctx->stream;

   if (begin)
   {
      pl.start = take_event(ctx);
      pl.stop = take_event(ctx);
      (void)hipEventRecord(pl.start, on);
   }
   else
   {
      (void)hipEventRecord(pl.stop, on);
      into.push_back(pl);
   }
}

int run_windowed(nfcgpu_ctx *ctx, uint32_t config, const std::vector<WindowedItem> &items, uint32_t stride);
int launch_sequential(nfcgpu_ctx *ctx, uint32_t config, const std::vector<WindowedItem> &items, uint32_t stride);

/* the same submission, `blockSamples` at a time (0: the context's block length) */
int run_in_blocks(nfcgpu_ctx *ctx, uint32_t config, const std::vector<WindowedItem> &items, uint32_t stride, uint32_t blockSamples = 0)
{
   uint32_t longest = 0;
   for (const WindowedItem &it: items)
      longest = it.count > longest ? it.count : longest;

   if (!blockSamples)
      blockSamples = ctx->blockSamples;

   int rc = NFCGPU_OK;
   ctx->inBlocks = true;

   for (uint64_t at = 0; at < longest && rc == NFCGPU_OK; at += blockSamples)
   {
      std::vector<WindowedItem> block;

      for (const WindowedItem &it: items)
      {
         if (it.count > at)
         {
            const uint64_t left = it.count - at;
            block.push_back(WindowedItem {it.slot, it.data + (size_t)at * nfc_sample_bytes(stride), (uint32_t)(left < blockSamples ? left : blockSamples)});
         }
      }

      rc = windowed_eligible(ctx, config, block) ? run_windowed(ctx, config, block, stride) : launch_sequential(ctx, config, block, stride);
   }

   ctx->inBlocks = false;
   return rc;
}

/* ------------------------------------------------------------------------------------------ */
/* the tail of a time-parallel submission                                                      */
/* ------------------------------------------------------------------------------------------ */

/* What is left of a submission once its first decode pass and the chain kernel behind it are queued: the later passes - a few
 * thousand lanes, then a few dozen, each pass as long as its longest lane at one wave's speed -, the final lanes, the finish and
 * the job read-back. The device is all but idle under it, so it is kept as a small resumable object: a submission may return to
 * its caller with the tail pending on the context, and the next one walks its own front (scan, seam rounds, planes) on a stream
 * of its own while it advances this tail whenever a host wait of that front returns (run_windowed). The states sit at the host
 * read-backs the pass loop has always had: the run list's length, the chain kernel's "again", the staging sink's control words,
 * the job table. A submission that is not deferred goes through the same states, waiting at each. */
struct WindowedTail
{
   enum State { RunList, Chain, Staging, Jobs };
   State state = RunList;
   bool deferred = false;          /* the submission has returned to its caller with this pending */
   uint32_t config = 0, stride = 0;
   std::vector<WindowedItem> items;
   NfcScanArgs A;
   NfcLaunch real, lanes;
   const NfcConfig *dCfg = nullptr;
   uint32_t *counters = nullptr;
   const void *dJobs = nullptr;    /* the job table of the buffer set the submission's front wrote */
   uint32_t nJobs = 0, nWindows = 0, windowBlocks = 0, firstWindowSlot = 0, finalLaneSlot = 0, pass = 0;
   uint64_t totalSamples = 0;
   ProfiledLaunch pw {nullptr, nullptr};
   std::vector<hipEvent_t> passEvents; /* fork / join events in flight; back to the pool once the pass has been waited for */
   bool sideRunning = false;       /* the side stream may be running kernels of the pass that the main stream does not wait for yet */
   hipEvent_t ready = nullptr;     /* recorded behind the read-back the state waits for */
   nfcgpu_ctx::StageSlot *slot = nullptr; /* staging slot of a host-resident submission: held until the tail is done */
   bool debugStages = false;
   std::chrono::steady_clock::time_point passBegan, stageBegan;
};

/* samples the pending tail's submission advances a slot's clock by (the host mirror follows when the tail completes) */
uint32_t tail_ahead(const nfcgpu_ctx *ctx, uint32_t slot)
{
   if (!ctx->tail || ctx->tail->items.empty())
      return 0u;

   /* (a pending tail is a uniform submission's: a contiguous range of slots in order) */
   const std::vector<WindowedItem> &items = ctx->tail->items;
   const uint32_t first = items.front().slot;

   if (slot >= first && slot - first < items.size() && items[slot - first].slot == slot)
      return items[slot - first].count;

   for (const WindowedItem &it: items)
      if (it.slot == slot)
         return it.count;

   return 0u;
}

/* one lane per slot: the carry lanes (and, at the end, the lanes that regenerate a job's final state) */
int tail_decode_slots(nfcgpu_ctx *ctx, WindowedTail &T, bool carry, uint32_t firstSlot, uint32_t slotCount, hipStream_t on)
{
   if (slotCount == 0)
      return NFCGPU_OK;

   NfcLaunch L = T.lanes;
   L.firstSlot = firstSlot;
   L.slotCount = slotCount;
   L.firstBlock = firstSlot / NFC_LANES;
   L.warmFront = carry ? 0u : NFC_WINDOW_WARM_FRONT;
   L.warmCorr = carry ? 0u : NFC_WINDOW_WARM_CORR;

   ProfiledLaunch wl {nullptr, nullptr};
   record_span(ctx, ctx->timedWave, wl, true, on);
   hipLaunchKernelGGL(NFC_BY_LAYOUT(T.A.stride, nfc_wave_kernel), dim3(slotCount), dim3(NFC_LANES), 0, on, T.dCfg, L, T.A, carry ? 0u : 2u); /* a wave per lane */
   record_span(ctx, ctx->timedWave, wl, false, on);
   HIP_TRY(ctx, hipGetLastError());
   ctx->stats.launches++;
   return NFCGPU_OK;
}

/* the speculative windows on the run list: persistent waves */
int tail_decode_windows(nfcgpu_ctx *ctx, WindowedTail &T, uint32_t runLanes)
{
   NfcLaunch L = T.lanes;
   L.warmFront = NFC_WINDOW_WARM_FRONT;
   L.warmCorr = NFC_WINDOW_WARM_CORR;

   ProfiledLaunch wl {nullptr, nullptr};
   record_span(ctx, ctx->timedWave, wl, true);
   hipLaunchKernelGGL(NFC_BY_LAYOUT(T.A.stride, nfc_wave_kernel), dim3(runLanes), dim3(NFC_LANES), 0, ctx->stream, T.dCfg, L, T.A, 1u); /* a wave per run-list entry */
   record_span(ctx, ctx->timedWave, wl, false);
   HIP_TRY(ctx, hipGetLastError());
   ctx->stats.launches++;
   return NFCGPU_OK;
}

/* the run list of the coming pass, and its length on the way to the host */
int tail_list(nfcgpu_ctx *ctx, WindowedTail &T)
{
   const NfcScanArgs &A = T.A;
   const NfcLaunch &lanes = T.lanes;
   uint32_t *counters = T.counters;
   const uint32_t pass = T.pass, windowBlocks = T.windowBlocks;
   const NfcConfig *dCfg = T.dCfg;

   T.passBegan = std::chrono::steady_clock::now();

   if (T.nWindows)
   {
      HIP_TRY(ctx, hipMemsetAsync(counters + 2, 0, 8, ctx->stream)); /* run list: count and next */
      if (!ctx->longFirst)
      {
         hipLaunchKernelGGL(nfc_window_lanes_kernel, dim3(windowBlocks), dim3(NFC_LANES), 0, ctx->stream, dCfg, A, lanes, pass, 0u, 0u, 0xFFFFFFFFu);
         HIP_TRY(ctx, hipGetLastError());
      }
      else
      {
         /* longest lanes first: classes of 65536 samples and more, then halving down to NFCGPU_LONG_FIRST, then the rest */
         uint32_t hi = 0xFFFFFFFFu, lo = 65536u > ctx->longFirst ? 65536u : ctx->longFirst;

         for (uint32_t order = 1u;; order = 2u)
         {
            hipLaunchKernelGGL(nfc_window_lanes_kernel, dim3(windowBlocks), dim3(NFC_LANES), 0, ctx->stream, dCfg, A, lanes, pass, order, lo, hi);
            HIP_TRY(ctx, hipGetLastError());

            if (lo == 0u)
               break;

            hi = lo;
            lo = lo / 2u >= ctx->longFirst ? lo / 2u : 0u;
         }
      }
      /* how many lanes the list holds: the later passes of a submission list a few thousand, then a few dozen, of its windows -
       * the launch gets a grid of the list's length, not of the submission's window count */
      HIP_TRY(ctx, hipMemcpyAsync(ctx->tailHost + 1, counters + 2, 4, hipMemcpyDeviceToHost, ctx->stream));
   }

   HIP_TRY(ctx, hipEventRecord(T.ready, ctx->stream));
   T.state = WindowedTail::RunList;
   return NFCGPU_OK;
}

/* has the read-back the tail waits for arrived? (`block`: wait for it) */
int tail_is_ready(nfcgpu_ctx *ctx, WindowedTail &T, bool block, bool *is)
{
#ifdef NFCGPU_EMULATED_TEST_BUILD
   /* (the emulated runtime's streams are synchronous: it has arrived) */
   (void)block;
   HIP_TRY(ctx, hipEventSynchronize(T.ready));
   *is = true;
#else
   if (block)
   {
      HIP_TRY(ctx, hipEventSynchronize(T.ready));
      *is = true;
   }
   else
   {
      const hipError_t q = hipEventQuery(T.ready);
      if (q != hipSuccess && q != hipErrorNotReady)
         return fail(ctx, NFCGPU_EHIP, "hipEventQuery(T.ready)", q);
      *is = q == hipSuccess;
   }
#endif
   return NFCGPU_OK;
}

/* one state of the tail, if what it waits for is there */
int tail_step(nfcgpu_ctx *ctx, WindowedTail &T, bool block, bool *done)
{
   NfcScanArgs &A = T.A;
   NfcLaunch &lanes = T.lanes;
   NfcLaunch &real = T.real;
   uint32_t *counters = T.counters;
   const uint32_t nJobs = T.nJobs, nWindows = T.nWindows, firstWindowSlot = T.firstWindowSlot, finalLaneSlot = T.finalLaneSlot;
   const uint64_t totalSamples = T.totalSamples;
   const NfcConfig *dCfg = T.dCfg;
   const std::vector<WindowedItem> &items = T.items;
   std::vector<hipEvent_t> &passEvents = T.passEvents;
   int rc;

   *done = false;

   {
      bool is = false;
      if ((rc = tail_is_ready(ctx, T, block, &is)))
         return rc;
      if (!is)
         return NFCGPU_OK;
   }

   const bool debugStages = T.debugStages;
   auto mark = [&](const char *what) {
      if (!debugStages)
         return;
      (void)hipStreamSynchronize(ctx->stream);
      const auto now = std::chrono::steady_clock::now();
      std::fprintf(stderr, "[nfcgpu] windowed stage %-10s %8.2f ms\n", what, std::chrono::duration<double, std::milli>(now - T.stageBegan).count());
      T.stageBegan = now;
   };

   switch (T.state)
   {
   case WindowedTail::RunList:
   {
      const uint32_t pass = T.pass;
      uint32_t runLanes = nWindows ? ctx->tailHost[1] : 0u;
      if (runLanes > nWindows)
         runLanes = nWindows;

      /* the carry lanes (later passes: those the chain kernel sent on): from the stream's own state, which has not
       * been touched */
      if (pass > 0)
      {
         hipLaunchKernelGGL(nfc_carry_lanes_kernel, dim3(nJobs), dim3(NFC_LANES), 0, ctx->stream, A, real, lanes, pass);
         HIP_TRY(ctx, hipGetLastError());
      }

      /* carry lanes and speculative lanes side by side: no lane looks at what another one is doing while it runs
       * (nfc_lane_handover), and the longest lane of either kind can be most of the submission */
      if (ctx->sideMode == 0 || nWindows == 0 || runLanes == 0)
      {
         /* nothing to run beside (or NFCGPU_SIDE_STREAM=0): one stream */
         if ((rc = tail_decode_slots(ctx, T, true, 0, nJobs, ctx->stream)))
            return rc;
         if (nWindows && runLanes && (rc = tail_decode_windows(ctx, T, runLanes)))
            return rc;
      }
      else
      {
         /* events of this pass only (never recorded again while a wait on them may be pending) */
         hipEvent_t fork = ctx->sideMode == 2 ? take_event(ctx) : ctx->forkEvent;
         hipEvent_t join = ctx->sideMode == 2 ? take_event(ctx) : ctx->joinEvent;

         if (ctx->sideMode == 2)
         {
            passEvents.push_back(fork);
            passEvents.push_back(join);
         }

         HIP_TRY(ctx, hipEventRecord(fork, ctx->stream));
         HIP_TRY(ctx, hipStreamWaitEvent(ctx->side, fork, 0));
         T.sideRunning = true;

         if ((rc = tail_decode_slots(ctx, T, true, 0, nJobs, ctx->side)))
            return rc;

         HIP_TRY(ctx, hipEventRecord(join, ctx->side));

         if (runLanes && (rc = tail_decode_windows(ctx, T, runLanes)))
            return rc;

         HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, join, 0));
         T.sideRunning = false; /* (the main stream now waits for it) */
      }

      HIP_TRY(ctx, hipMemsetAsync(counters + 1, 0, 4, ctx->stream));
      hipLaunchKernelGGL(nfc_chain_kernel, dim3((nJobs + 63) / 64), dim3(64), 0, ctx->stream, A, lanes, nJobs >= NFC_LANES ? ctx->maxPasses : ctx->maxPassesFew);
      HIP_TRY(ctx, hipGetLastError());

      HIP_TRY(ctx, hipMemcpyAsync(ctx->tailHost, counters + 1, 4, hipMemcpyDeviceToHost, ctx->stream));
      HIP_TRY(ctx, hipEventRecord(T.ready, ctx->stream));
      T.state = WindowedTail::Chain;
      return NFCGPU_OK;
   }

   case WindowedTail::Chain:
   {
      const uint32_t pass = T.pass;
      const uint32_t again = ctx->tailHost[0];
      const auto passBegan = T.passBegan;

#if defined(NFCGPU_TUNING_KNOBS) || defined(NFCGPU_EMULATED_TEST_BUILD)
      /* (the tuning build: NFCGPU_DUMP_WINDOWS=<file> - the pieces of the first pass as they ended, five words each: job, start,
       * sample from which the piece was live, first sample not consumed, how it ended; profiles/tools/r06/item5_pieces_ab.py) */
      if (pass == 0 && nWindows)
         if (const char *dumpTo = std::getenv("NFCGPU_DUMP_WINDOWS"))
         {
            std::vector<NfcWindow> ws(nWindows);
            HIP_TRY(ctx, hipMemcpy(ws.data(), (const NfcWindow *)ctx->wWindows.ptr + firstWindowSlot, sizeof(NfcWindow) * ws.size(), hipMemcpyDeviceToHost));
            if (FILE *f = std::fopen(dumpTo, "ab"))
            {
               for (const NfcWindow &w: ws)
               {
                  const uint32_t rec[5] = {w.job, w.start, w.activate, w.stop, w.retired};
                  std::fwrite(rec, 4, 5, f);
               }
               std::fclose(f);
            }
         }
#endif

      if (debugStages)
      {
         uint32_t ls[3] = {0, 0, 0}, tilesTaken = 0;
         HIP_TRY(ctx, hipMemcpy(ls, counters + 4, 12, hipMemcpyDeviceToHost));
         HIP_TRY(ctx, hipMemcpy(&tilesTaken, counters + 10, 4, hipMemcpyDeviceToHost));
         HIP_TRY(ctx, hipMemsetAsync(counters + 4, 0, 12, ctx->stream));
         HIP_TRY(ctx, hipMemsetAsync(counters + 10, 0, 4, ctx->stream));
         HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
         const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - passBegan).count();
         {
            /* (a library built with -DNFC_WAVE_PROFILE: shader cycles per phase of the wave decoder, nfc_wave.hpp) */
            uint32_t prof[16] = {0};
            HIP_TRY(ctx, hipMemcpy(prof, counters + 16, 64, hipMemcpyDeviceToHost));
            HIP_TRY(ctx, hipMemsetAsync(counters + 16, 0, 64, ctx->stream));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            uint64_t all = 0;
            for (uint32_t v: prof)
               all += v;
            if (all)
               std::fprintf(stderr, "[nfcgpu]    wave cycles x 2^10: boundary %u, tile load %u, values %u, search gates %u, commit %u, step %u, search step %u, set-up %u, "
                                    "prologue %u, locked gates %u, detectors shown their records %u (gates after it: %u), between %u, step: state in %u, machine %u, state out %u\n", prof[0], prof[1], prof[2], prof[3], prof[4], prof[5],
                            prof[6], prof[7], prof[8], prof[9], prof[10], prof[15], prof[11], prof[12], prof[13], prof[14]);
         }
         if (std::atoi(std::getenv("NFCGPU_WINDOW_DEBUG")) >= 2 && nWindows)
         {
            /* the lanes of the first stream as the pass left them */
            std::vector<NfcScanJob> jb(1);
            HIP_TRY(ctx, hipMemcpy(jb.data(), ctx->wJobs.ptr, sizeof(NfcScanJob), hipMemcpyDeviceToHost));
            std::vector<NfcWindow> ws(jb[0].windows);
            if (!ws.empty())
               HIP_TRY(ctx, hipMemcpy(ws.data(), (const NfcWindow *)ctx->wWindows.ptr + jb[0].firstWindow, sizeof(NfcWindow) * ws.size(), hipMemcpyDeviceToHost));
            for (size_t i = 0; i < ws.size(); i++)
               std::fprintf(stderr, "[nfcgpu]    lane %3zu: start %8u live from %8u verify %8u stop %8u (%7u samples) retired %u to %3u, rerun %u live %u pub %u\n", i, ws[i].start,
                            ws[i].activate, ws[i].verify, ws[i].stop, ws[i].stop - ws[i].start, ws[i].retired, ws[i].handTo - jb[0].firstWindow, ws[i].rerun, ws[i].live,
                            ws[i].pubState);
         }
         if (std::atoi(std::getenv("NFCGPU_WINDOW_DEBUG")) >= 5 && nWindows)
         {
            /* why lanes are sent round again: what each lane marked for another run assumed (carry) against what it is told to assume (want) */
            std::vector<NfcScanJob> jb(nJobs);
            HIP_TRY(ctx, hipMemcpy(jb.data(), ctx->wJobs.ptr, sizeof(NfcScanJob) * nJobs, hipMemcpyDeviceToHost));
            uint32_t shown = 0;
            {
               /* tally over every lane marked: which fields of its assumption are to change */
               std::vector<NfcWindow> all(nWindows);
               HIP_TRY(ctx, hipMemcpy(all.data(), (const NfcWindow *)ctx->wWindows.ptr + firstWindowSlot, sizeof(NfcWindow) * all.size(), hipMemcpyDeviceToHost));
               uint64_t n[10] = {0}, samples = 0, over[4] = {0, 0, 0, 0};
               uint32_t longest = 0;
               for (const NfcWindow &w: all)
               {
                  if (!w.rerun)
                     continue;
                  const NfcCarry &a = w.carry, &b = w.want;
                  bool tim = false, wait = false;
                  for (int t = 0; t < 4; t++)
                  {
                     tim = tim || a.tim[t].lastCommand != b.tim[t].lastCommand || a.tim[t].maxFrameSize != b.tim[t].maxFrameSize || a.tim[t].protoGuardTime != b.tim[t].protoGuardTime;
                     wait = wait || a.tim[t].protoWaitingTime != b.tim[t].protoWaitingTime;
                  }
                  const bool chained = a.chainedA != b.chainedA, carrier = (a.carrierOn != 0) != (b.carrierOn != 0) || (a.carrierOff != 0) != (b.carrierOff != 0);
                  const bool emit = a.emitValid != b.emitValid || a.emitClock != b.emitClock;
                  const bool pulses = a.pulsesF[0] != b.pulsesF[0] || a.pulsesF[1] != b.pulsesF[1] || std::memcmp(a.thrF, b.thrF, 8) != 0;
                  const bool records = std::memcmp(&a.search, &b.search, sizeof(a.search)) != 0;
                  n[0]++; n[1] += chained; n[2] += carrier; n[3] += emit; n[4] += tim; n[5] += wait; n[6] += pulses; n[7] += records;
                  n[8] += !(chained || carrier || emit || tim || wait || pulses || records) ? 1 : 0;
                  n[9] += (chained && !(carrier || tim || wait || pulses || records)) ? 1 : 0;
                  samples += w.stop - w.start;
                  const uint32_t len = w.stop - w.start;
                  longest = len > longest ? len : longest;
                  over[0] += len >= 65536u; over[1] += len >= 131072u; over[2] += len >= 196608u; over[3] += len >= 262144u;
               }
               {
                  /* the longest of them, and the streams they belong to */
                  std::vector<const NfcWindow *> byLen;
                  for (const NfcWindow &w: all)
                     if (w.rerun)
                        byLen.push_back(&w);
                  std::sort(byLen.begin(), byLen.end(), [](const NfcWindow *a, const NfcWindow *b) { return a->stop - a->start > b->stop - b->start; });
                  for (size_t i = 0; i < byLen.size() && i < 6; i++)
                     std::fprintf(stderr, "[nfcgpu]    long lane: job %u start %u activate %u stop %u (%u samples) retired %u handTo %u noHand %u\n", byLen[i]->job, byLen[i]->start, byLen[i]->activate,
                                  byLen[i]->stop, byLen[i]->stop - byLen[i]->start, byLen[i]->retired, byLen[i]->handTo, byLen[i]->noHand);
               }
               std::fprintf(stderr, "[nfcgpu]    ... of them %llu ran 65536 samples and more, %llu 131072+, %llu 196608+, %llu 262144+; the longest %u\n",
                            (unsigned long long)over[0], (unsigned long long)over[1], (unsigned long long)over[2], (unsigned long long)over[3], longest);
               std::fprintf(stderr, "[nfcgpu]    lanes to run again %llu (%llu samples as they last ran): chainedA %llu (and nothing else but the carrier record: %llu), carrier on/off %llu, "
                                    "carrier record %llu, command / frame size / guard %llu, waiting time %llu, NFC-F pulse memory %llu, detector records %llu, same assumption (sent on past a hand-over) %llu\n",
                            (unsigned long long)n[0], (unsigned long long)samples, (unsigned long long)n[1], (unsigned long long)n[9], (unsigned long long)n[2], (unsigned long long)n[3],
                            (unsigned long long)n[4], (unsigned long long)n[5], (unsigned long long)n[6], (unsigned long long)n[7], (unsigned long long)n[8]);
            }
            for (uint32_t j = 0; j < nJobs && shown < 24 && pass >= 3; j++)
            {
               if (!(jb[j].status & NFC_JOB_RERUN) || !jb[j].windows)
                  continue;
               std::vector<NfcWindow> ws(jb[j].windows);
               HIP_TRY(ctx, hipMemcpy(ws.data(), (const NfcWindow *)ctx->wWindows.ptr + jb[j].firstWindow, sizeof(NfcWindow) * ws.size(), hipMemcpyDeviceToHost));
               for (size_t i = 0; i < ws.size(); i++)
               {
                  const NfcWindow &w = ws[i];
                  if (!w.rerun)
                     continue;
                  shown++;
                  std::fprintf(stderr, "[nfcgpu]    job %u lane %zu/%zu start %u stop %u retired %u noHand %u handTo %u:", j, i, ws.size(), w.start, w.stop, w.retired, w.noHand, w.handTo);
                  const NfcCarry &a = w.carry, &b = w.want;
                  if (a.chainedA != b.chainedA) std::fprintf(stderr, " chainedA %u->%u", a.chainedA, b.chainedA);
                  if ((a.carrierOn != 0) != (b.carrierOn != 0)) std::fprintf(stderr, " carrierOn %u->%u", a.carrierOn, b.carrierOn);
                  if ((a.carrierOff != 0) != (b.carrierOff != 0)) std::fprintf(stderr, " carrierOff %u->%u", a.carrierOff, b.carrierOff);
                  if (a.emitValid != b.emitValid || a.emitClock != b.emitClock) std::fprintf(stderr, " emit %u/%u->%u/%u (tracked %u)", a.emitValid, a.emitClock, b.emitValid, b.emitClock, w.tracked);
                  for (int t = 0; t < 4; t++)
                  {
                     if (a.tim[t].lastCommand != b.tim[t].lastCommand) std::fprintf(stderr, " cmd[%d] %u->%u", t, a.tim[t].lastCommand, b.tim[t].lastCommand);
                     if (a.tim[t].maxFrameSize != b.tim[t].maxFrameSize) std::fprintf(stderr, " maxFrame[%d] %u->%u", t, a.tim[t].maxFrameSize, b.tim[t].maxFrameSize);
                     if (a.tim[t].protoGuardTime != b.tim[t].protoGuardTime) std::fprintf(stderr, " guard[%d] %u->%u", t, a.tim[t].protoGuardTime, b.tim[t].protoGuardTime);
                     if (a.tim[t].protoWaitingTime != b.tim[t].protoWaitingTime) std::fprintf(stderr, " wait[%d] %u->%u", t, a.tim[t].protoWaitingTime, b.tim[t].protoWaitingTime);
                  }
                  for (int i2 = 0; i2 < 2; i2++)
                     if (a.pulsesF[i2] != b.pulsesF[i2] || std::memcmp(&a.thrF[i2], &b.thrF[i2], 4)) std::fprintf(stderr, " F%d pulses %u->%u thr %g->%g", i2, a.pulsesF[i2], b.pulsesF[i2], a.thrF[i2], b.thrF[i2]);
                  if (std::memcmp(&a.search, &b.search, sizeof(a.search))) std::fprintf(stderr, " records");
                  std::fprintf(stderr, "\n");
               }
            }
         }
         /* (lane-steps: samples handled one by one by the step machine; tiles: what the lanes took in all, warm-ups included) */
         std::fprintf(stderr, "[nfcgpu] windowed pass %u: %u lanes, %u tiles of %llu (%.1f tiles per us), %llu lane-steps (%.2f per sample), longest lane %u steps, %u streams unsettled, %.1f ms\n",
                      pass, ls[2], tilesTaken, (unsigned long long)((totalSamples + NFC_SCAN_TILE - 1) / NFC_SCAN_TILE), ms > 0.0 ? (double)tilesTaken / (ms * 1000.0) : 0.0,
                      (unsigned long long)ls[0] * NFC_SCAN_TILE, (double)ls[0] * NFC_SCAN_TILE / (double)totalSamples, ls[1] * NFC_SCAN_TILE, again, ms);
      }

      for (hipEvent_t e: passEvents)
         ctx->eventPool.push_back(e); /* (the stream has been synchronised above) */
      passEvents.clear();

      ctx->stats.window_passes++;
      T.pass++;

      if (again && nWindows)
         return tail_list(ctx, T);

      mark("passes");

      /* a library whose wave decoder was built with -DNFC_WAVE_VERIFY (Makefile: libnfcgpu_verify.so) has decoded every tile twice
       * and counted (csrc/nfc_wave.hip); a product build leaves the words at zero */
      if (std::getenv("NFCGPU_WAVE_VERIFY_REPORT"))
      {
         uint32_t v[4] = {0, 0, 0, 0};
         HIP_TRY(ctx, hipMemcpyAsync(v, counters + 12, 16, hipMemcpyDeviceToHost, ctx->stream));
         HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
         std::fprintf(stderr, "[nfcgpu] wave verify: %u tiles decoded twice (bulk paths / step machine alone), %u differ", v[0], v[1]);
         if (v[1])
            std::fprintf(stderr, " (the first at stream position %u of lane slot %u)", v[2], v[3]);
         std::fprintf(stderr, "\n");
      }

      /* The lanes chain their frame records in a staging sink that is sized from an estimate and written by every lane of
       * every pass, live in the end or not. Should it have run full, frames of live lanes may be among the ones that did not
       * fit: nothing of the streams has been touched yet, so the submission is decoded by the sequential kernels instead. */
      HIP_TRY(ctx, hipMemcpyAsync(ctx->tailHost + 2, ctx->vSinkCtl.ptr, 8, hipMemcpyDeviceToHost, ctx->stream));
      HIP_TRY(ctx, hipEventRecord(T.ready, ctx->stream));
      T.state = WindowedTail::Staging;
      return NFCGPU_OK;
   }

   case WindowedTail::Staging:
   {
      if (ctx->tailHost[3])
      {
         HIP_TRY(ctx, hipMemsetAsync(ctx->vSinkCtl.ptr, 0, 16, ctx->stream));
         ctx->stats.fallback_streams += nJobs;
         *done = true;
         return launch_sequential(ctx, T.config, items, T.stride);
      }

      /* the state a stream is left in: its last lane's, run once more with storage of its own */
      hipLaunchKernelGGL(nfc_final_lanes_kernel, dim3((nJobs + 63) / 64), dim3(64), 0, ctx->stream, dCfg, A, lanes);
      HIP_TRY(ctx, hipGetLastError());

      if ((rc = tail_decode_slots(ctx, T, false, finalLaneSlot, nJobs, ctx->stream)))
         return rc;

      record_span(ctx, ctx->timedWindow, T.pw, false);

      hipLaunchKernelGGL(nfc_finish_kernel, dim3(nJobs), dim3(NFC_LANES), 0, ctx->stream, A, real, lanes);
      HIP_TRY(ctx, hipGetLastError());

      /* (the job table comes back into pinned memory: a copy into pageable memory would hold the host until it is done) */
      if (ctx->tailJobsBytes < sizeof(NfcScanJob) * nJobs)
      {
         if (ctx->tailJobs)
            (void)hipHostFree(ctx->tailJobs);
         ctx->tailJobs = nullptr;
         ctx->tailJobsBytes = 0;
         if (hipHostMalloc((void **)&ctx->tailJobs, sizeof(NfcScanJob) * nJobs, hipHostMallocDefault) != hipSuccess)
         {
            (void)hipGetLastError();
            ctx->tailJobs = nullptr;
            return fail(ctx, NFCGPU_ENOMEM, "pinned buffer for the job table of the time-parallel path could not be allocated");
         }
         ctx->tailJobsBytes = sizeof(NfcScanJob) * nJobs;
      }

      HIP_TRY(ctx, hipMemcpyAsync(ctx->tailJobs, T.dJobs, sizeof(NfcScanJob) * nJobs, hipMemcpyDeviceToHost, ctx->stream));
      HIP_TRY(ctx, hipEventRecord(T.ready, ctx->stream));
      T.state = WindowedTail::Jobs;
      return NFCGPU_OK;
   }

   case WindowedTail::Jobs:
   {
      const NfcScanJob *jobs = ctx->tailJobs;

      mark("finish");

      if (debugStages && std::atoi(std::getenv("NFCGPU_WINDOW_DEBUG")) >= 3 && nWindows)
      {
         /* how much of what the speculative lanes decoded ended up in the stream (the rest was overrun by a lane that could
          * not hand over, or decoded again in a later pass) */
         std::vector<NfcWindow> ws(nWindows);
         HIP_TRY(ctx, hipMemcpy(ws.data(), (const NfcWindow *)ctx->wWindows.ptr + firstWindowSlot, sizeof(NfcWindow) * ws.size(), hipMemcpyDeviceToHost));
         uint64_t all = 0, live = 0, liveLanes = 0;
         for (const NfcWindow &w: ws)
         {
            all += w.stop - w.start;
            if (w.live)
            {
               live += w.stop - w.start;
               liveLanes++;
            }
         }
         std::fprintf(stderr, "[nfcgpu] speculative lanes: %zu, %llu samples as they last ran; live in the end: %llu lanes, %llu samples (%.1f %%); submission: %llu samples\n", ws.size(),
                      (unsigned long long)all, (unsigned long long)liveLanes, (unsigned long long)live, all ? 100.0 * (double)live / (double)all : 0.0, (unsigned long long)totalSamples);
      }

      ctx->stats.windows += nWindows + nJobs;
      ctx->stats.samples += totalSamples;
      ctx->dirty = true;

      std::vector<WindowedItem> fallback;

      for (uint32_t j = 0; j < nJobs; j++)
      {
         if (jobs[j].status & NFC_JOB_INVALID)
            fallback.push_back(items[j]);
         else
         {
            ctx->streams[items[j].slot].clock += items[j].count;
            ctx->stats.windowed_streams++;
         }
      }

      ctx->stats.fallback_streams += fallback.size();

      mark("return");

      if (!fallback.empty())
      {
         ctx->stats.samples -= 0; /* launch_demod counts the samples of the streams it decodes */
         uint64_t again = 0;
         for (const WindowedItem &it: fallback)
            again += it.count;
         ctx->stats.samples -= again;
         *done = true;
         return launch_sequential(ctx, T.config, fallback, T.stride);
      }

      *done = true;
      return NFCGPU_OK;
   }
   }

   return NFCGPU_OK;
}

/* advance the pending tail by a state if it can go on (`block`: wait until it can); done or failed, it leaves the context */
int tail_advance(nfcgpu_ctx *ctx, bool block)
{
   WindowedTail *T = ctx->tail;
   if (!T)
      return NFCGPU_OK;

   bool done = false;
   const int rc = tail_step(ctx, *T, block, &done);

   if (rc != NFCGPU_OK || done)
   {
      /* Whatever way the tail ends while the side stream may still be running kernels of a pass (a launch that failed after the
       * fork, an event that could not be recorded): the side stream is waited for before anyone reuses the staging slot or the
       * lane buffers it reads, and the events of the pass go back to the pool. */
      if (T->sideRunning)
         (void)hipStreamSynchronize(ctx->side);
      if (rc != NFCGPU_OK)
         (void)hipStreamSynchronize(ctx->stream);
      for (hipEvent_t e: T->passEvents)
         ctx->eventPool.push_back(e);
      if (T->ready)
         ctx->eventPool.push_back(T->ready);
      if (T->slot)
         stage_release(ctx, T->slot);
      ctx->tail = nullptr;
      delete T;
   }

   return rc;
}

/* complete the pending tail, finish included: what every entry point does first, a submission that runs its front under the
 * tail excepted. An error met in the tail is returned here, by the call that completes it. */
int settle_tail(nfcgpu_ctx *ctx)
{
   while (ctx->tail)
   {
      const int rc = tail_advance(ctx, true);
      if (rc)
         return rc;
   }

   return NFCGPU_OK;
}

/* ... as the first thing an entry point of the C ABI does */
int settle_entry(nfcgpu_ctx *ctx)
{
   if (!ctx->tail)
      return NFCGPU_OK;

   HIP_TRY(ctx, hipSetDevice(ctx->device));
   return settle_tail(ctx);
}

#define SETTLE_FIRST(ctx)                            \
   do                                                \
   {                                                 \
      if (ctx)                                       \
      {                                              \
         const int settled__ = settle_entry(ctx);    \
         if (settled__)                              \
            return settled__;                        \
      }                                              \
   } while (0)

/* the front of the new submission under the pending tail? Only when it continues the very streams of the pending one. */
bool may_overlap(nfcgpu_ctx *ctx, uint32_t config, const std::vector<WindowedItem> &items)
{
   const WindowedTail *T = ctx->tail;

   if (!T || !T->deferred || !ctx->pipeline || ctx->noSecondSet || ctx->inBlocks || !ctx->front || !ctx->wShadow.ptr || T->config != config || T->items.size() != items.size())
      return false;

   for (size_t i = 0; i < items.size(); i++)
      if (items[i].slot != T->items[i].slot)
         return false;

   return true;
}

/* the two sets of the buffers a front writes and a tail still reads change places */
void swap_front_sets(nfcgpu_ctx *ctx)
{
   nfcgpu_ctx::DevBuf *mine[] = {&ctx->wRepairs, &ctx->wJobs, &ctx->wChunks, &ctx->wPoints, &ctx->wSeams, &ctx->wChunkEdge, &ctx->wTiles, &ctx->wTileStats, &ctx->wCounters,
                                 &ctx->wRepairsEnv, &ctx->wPlanes, &ctx->wPlaneChunks, &ctx->wPlanesStale};

   for (size_t i = 0; i < sizeof(mine) / sizeof(mine[0]); i++)
      std::swap(*mine[i], ctx->otherSet[i]);
}

/* A time-parallel submission from its plan to the hand-off to its tail: what the stages below read and write. It lives on the
 * stack of run_windowed; the stages are free functions in the order they run, and what is left of the submission afterwards is
 * copied into its WindowedTail. */
struct WindowedSubmission
{
   /* what was submitted */
   const uint32_t config, stride;
   const std::vector<WindowedItem> &items;
   const NfcConfig &cfg;
   const uint32_t nJobs;

   /* NFCGPU_WINDOW_DEBUG: where the time of a submission goes (synchronises at every mark); its value is how much else is shown */
   const bool debugStages;
   const int debugLevel;
   std::chrono::steady_clock::time_point stageBegan; /* (the stage log counts the host's tables from the call's entry) */

   bool under = false;  /* the front runs under the pending tail */
   bool routed = false; /* a stage has handed the whole submission to somebody else (blocks, quarters, the sequential kernels): its result is the call's */

   /* the plan: plan_scan_params, plan_tables */
   NfcScanParams sp;
   std::vector<NfcScanJob> jobs; /* (uploaded by the front; a small submission's are read back in its first seam round, counts of busy tiles filled in) */
   std::vector<NfcScanChunk> chunks;
   uint32_t nChunks = 0, tiles = 0, points = 0, tilesMost = 0, tilesGridY = 0;
   uint64_t totalSamples = 0;
   uint32_t finalLaneSlot = 0, firstWindowSlot = 0;

   /* what the kernels are given: fill_scan_args, then the front (planes, planesStale, states) and the back (lanes, save area) */
   NfcScanArgs A;
   const NfcConfig *dCfg = nullptr;
   uint32_t *counters = nullptr;

   /* the back */
   uint32_t nWindows = 0;
   bool shadows = false; /* shadow states have been asked for: the next submission may run its front under this one's tail */
};

/* the stage log: the stream is waited for and the time since the mark before printed */
void mark_stage(nfcgpu_ctx *ctx, WindowedSubmission &W, const char *what)
{
   if (!W.debugStages)
      return;
   (void)hipStreamSynchronize(ctx->stream);
   const auto now = std::chrono::steady_clock::now();
   std::fprintf(stderr, "[nfcgpu] windowed stage %-10s %8.2f ms\n", what, std::chrono::duration<double, std::milli>(now - W.stageBegan).count());
   W.stageBegan = now;
}

/* A work buffer the device cannot give (NFCGPU_ENOMEM from grow()) is not the end of a submission as long as nothing of the
 * streams has been touched - which holds up to the finish: the scan and the lanes only read the streams' state. The
 * submission is then decoded a quarter of its length at a time (a quarter of every work buffer), and if that does not fit
 * either by the sequential kernels, which need none. Any other error is the caller's.
 *
 * Reads the items; writes W.routed. Queues nothing itself: the submission is whoever it is handed to's. */
int without_the_memory(nfcgpu_ctx *ctx, WindowedSubmission &W, int code)
{
   W.routed = true;

   if (code != NFCGPU_ENOMEM)
      return code;

   (void)hipGetLastError();

   uint32_t longest = 0;
   for (const WindowedItem &it: W.items)
      longest = it.count > longest ? it.count : longest;

   const uint32_t quarter = longest / 4u / NFC_SCAN_POINT * NFC_SCAN_POINT;

   if (!ctx->inBlocks && quarter >= 65536u && quarter >= ctx->windowedMinSamples)
      return run_in_blocks(ctx, W.config, W.items, W.stride, quarter);

   ctx->stats.fallback_streams += W.nJobs;
   return launch_sequential(ctx, W.config, W.items, W.stride);
}

/* ---- the plan: host work alone, nothing is queued ---- */

/* The scan parameters (W.sp): thresholds from the configuration, chunk and warm-up lengths from the context's settings and the
 * submission's size. Reads W.cfg and the items. */
void plan_scan_params(nfcgpu_ctx *ctx, WindowedSubmission &W)
{
   const NfcConfig &cfg = W.cfg;
   const std::vector<WindowedItem> &items = W.items;
   NfcScanParams &sp = W.sp;

   float corr = 3.0e38f;
   if (cfg.enabled & 1u) corr = cfg.corrThreshold[0] < corr ? cfg.corrThreshold[0] : corr;
   if (cfg.enabled & 4u) corr = cfg.corrThreshold[2] < corr ? cfg.corrThreshold[2] : corr;
   if (cfg.enabled & 8u) corr = cfg.corrThreshold[3] < corr ? cfg.corrThreshold[3] : corr;
   sp.rangeK = corr < 1.0e30f ? 0.49f * corr : 3.0e38f;
   sp.edgeK = (cfg.enabled & 2u) ? 0.99f * cfg.minDepth[1] : 3.0e38f;
   float deep = 1.0f;
   for (int t = 0; t < 4; t++)
      if ((cfg.enabled >> t) & 1u)
         deep = cfg.maxDepth[t] < deep ? cfg.maxDepth[t] : deep;
   sp.deepK = 0.98f * deep;
   sp.chunkSamples = ctx->scanChunk;
   sp.warmSamples = ctx->scanWarm;
   sp.soloSamples = ctx->soloSamples;
   sp.offGridAlone = 1u;

   /* Every chunk pays the warm-up again, so chunks should be as long as the machine allows: one lane per chunk, and
    * 131072 lanes (256 CUs x 4 SIMDs x 2 waves of the scan kernel's 204 registers x 64) are resident at a time.
    * Measured on 4096 streams x 2^20 idle samples: 8192 -> 1347, 16384 -> 1673, 32768 -> 1906 GB/s. */
   if (!ctx->scanChunkFixed)
   {
      uint64_t total = 0;
      for (const WindowedItem &it: items)
         total += it.count;

      /* (round 4: a sixteenth of that is enough lanes. What a submission of 2^29 samples - 512 busy streams, an eighth of
       * config 5 - pays for are the rounds of second walks, a launch and a trip to the host each, and a chain of chunks that
       * inherit a wrong envelope from each other is as many rounds as it has chunks: 27 rounds of 4096-sample chunks, 8 of
       * 32768. 512 / 1024 dense streams x 2^20: 352 -> 321 ms per step.) */
      uint64_t chunk = total / ctx->scanLanes / NFC_SCAN_POINT * NFC_SCAN_POINT;
      if (chunk > 32768u)
         chunk = 32768u;
      if (chunk > sp.chunkSamples)
         sp.chunkSamples = (uint32_t)chunk;

      /* A small submission is one a caller waits for (a capture, a receiver's block): what counts is the time of the
       * longest walk, chunk + warm-up at ~0.4 us per sample and lane. Shorter chunks and a warm-up that just covers the
       * slowest recurrence (the average: 0.995^k) cut it; seams that do not verify cost a short second walk now. */
      if (total <= (4u << 20))
      {
         if (sp.chunkSamples > 4096u)
            sp.chunkSamples = 4096u;
         if (sp.warmSamples > 3072u)
            sp.warmSamples = 3072u;
      }
   }
}

/* Job and chunk tables (W.jobs, W.chunks) with the lane cut, and the sizes everything after them is dimensioned by: tiles,
 * points, chunks, samples, the lane slots, the y extent of a grid over tiles. Reads the items and W.sp. */
void plan_tables(nfcgpu_ctx *ctx, WindowedSubmission &W)
{
   const std::vector<WindowedItem> &items = W.items;
   const NfcScanParams &sp = W.sp;
   const uint32_t nJobs = W.nJobs;
   std::vector<NfcScanJob> &jobs = W.jobs;
   std::vector<NfcScanChunk> &chunks = W.chunks;
   uint32_t &tiles = W.tiles, &points = W.points, &tilesMost = W.tilesMost;
   uint64_t &totalSamples = W.totalSamples;

   jobs.resize(nJobs);

   for (uint32_t j = 0; j < nJobs; j++)
   {
      NfcScanJob &job = jobs[j];
      std::memset(&job, 0, sizeof(job));
      job.data = items[j].data;
      job.count = items[j].count;
      job.slot = items[j].slot;
      job.firstChunk = (uint32_t)chunks.size();
      job.chunks = (job.count + sp.chunkSamples - 1) / sp.chunkSamples;
      job.firstTile = tiles;
      job.firstPoint = points;
      tiles += (job.count + NFC_SCAN_TILE - 1) / NFC_SCAN_TILE;
      tilesMost = std::max(tilesMost, (job.count + NFC_SCAN_TILE - 1) / NFC_SCAN_TILE);
      points += job.count / NFC_SCAN_POINT + 1;
      totalSamples += job.count;

      for (uint32_t k = 0; k < job.chunks; k++)
         chunks.push_back(NfcScanChunk {j, k});
   }

   /* Lanes inside busy signal: NFC_WINDOW_CUT samples apart when the submission is small (every lane is parallelism),
    * further apart - fewer warm-ups, fewer hand-overs to go wrong - when that still leaves several lanes per wave slot
    * of the machine (NFCGPU_LANES_WANTED, default 16384 = 8 per slot of 256 CUs x 8 waves) */
   {
      uint64_t cut = ctx->lanesWanted ? totalSamples / ctx->lanesWanted : 0u;
      cut = cut / NFC_SCAN_POINT * NFC_SCAN_POINT;
      cut = cut < NFC_WINDOW_CUT ? NFC_WINDOW_CUT : (cut > ctx->cutMax ? ctx->cutMax : cut);

      for (NfcScanJob &job: jobs)
         job.cut = (uint32_t)cut;
   }

   W.nChunks = (uint32_t)chunks.size();
   W.finalLaneSlot = (nJobs + NFC_LANES - 1) / NFC_LANES * NFC_LANES;
   W.firstWindowSlot = 2 * W.finalLaneSlot;

   /* (a grid has at most 65535 blocks in y: beyond 2^24 tiles in one job the kernel strides) */
   W.tilesGridY = (tilesMost + 255) / 256 > 65535u ? 65535u : (tilesMost + 255) / 256;
}

/* the front-end planes: 16 bytes per sample of the submission, whole tiles (64 GiB for 4096 streams x 2^20) */
size_t planes_bytes(const WindowedSubmission &W)
{
   return (size_t)W.tiles * NFC_SCAN_TILE * 16u;
}

/* room for the planes, for a list of `listed` chunks or pieces to walk for them and, `stale`, for the marks of the chunks whose start
 * state is rewritten under a walk beside the rounds. Grows ctx->wPlanes, wPlaneChunks, wPlanesStale; queues nothing. */
int grow_planes(nfcgpu_ctx *ctx, const WindowedSubmission &W, size_t listed, bool stale)
{
   int r;
   if ((r = grow(ctx, ctx->wPlanes, planes_bytes(W))) || (r = grow(ctx, ctx->wPlaneChunks, sizeof(NfcScanChunk) * listed)))
      return r;
   return stale ? grow(ctx, ctx->wPlanesStale, 4u * (size_t)W.nChunks) : NFCGPU_OK;
}

/* The buffers the front writes and the tail still reads. Under a pending tail the front takes the second set of them (grown
 * here to everything the front may ask for, so that nothing is grown while it runs); a second set the device cannot give
 * means no overlap for this context - never the fallbacks of without_the_memory.
 *
 * Reads the sizes of the plan; grows the current front set (`all`: the planes' buffers too, as large as any way through the front
 * may ask for them); queues nothing. */
int grow_front(nfcgpu_ctx *ctx, const WindowedSubmission &W, bool all)
{
   const uint32_t nJobs = W.nJobs, nChunks = W.nChunks, tiles = W.tiles, points = W.points;
   int r;
   if ((r = grow(ctx, ctx->wJobs, sizeof(NfcScanJob) * nJobs)) || (r = grow(ctx, ctx->wChunks, sizeof(NfcScanChunk) * nChunks)) ||
       (r = grow(ctx, ctx->wPoints, sizeof(NfcScanPoint) * (size_t)points)) || (r = grow(ctx, ctx->wSeams, sizeof(NfcScanSeam) * nChunks)) ||
       (r = grow(ctx, ctx->wChunkEdge, 4 * (size_t)nChunks)) || (r = grow(ctx, ctx->wTiles, 4 * (size_t)tiles)) ||
       (r = grow(ctx, ctx->wTileStats, sizeof(NfcScanTile) * (size_t)tiles)) ||
       (r = grow(ctx, ctx->wCounters, 256)) || (r = grow(ctx, ctx->wRepairs, sizeof(NfcScanChunk) * nChunks)) ||
       (r = grow(ctx, ctx->wRepairsEnv, sizeof(NfcScanChunk) * nChunks)))
      return r;
   return all ? grow_planes(ctx, W, std::max(nChunks, points), true) : NFCGPU_OK;
}

/* A front under the pending tail takes the second buffer set (the sets change places: the context's members are the front's from
 * here on). A set the device cannot give: the sets change back, the tail is completed, W.under is dropped and - out of memory -
 * the context stops asking (noSecondSet), giving back what it got. Returns an error only for what ends the call. Queues nothing;
 * waits for the tail's streams when it gives up. */
int take_second_set(nfcgpu_ctx *ctx, WindowedSubmission &W)
{
   swap_front_sets(ctx);
   ctx->growingSecond = true;
   int rc = grow_front(ctx, W, true);
   ctx->growingSecond = false;

   if (rc)
   {
      (void)hipGetLastError();
      swap_front_sets(ctx);
      W.under = false;
      if (rc == NFCGPU_ENOMEM)
         ctx->noSecondSet = true;
      const int settled = settle_tail(ctx);

      /* (what was given of the second set before the device ran out goes back: it must not be what a later growth of the lane
       * buffers finds missing) */
      if (ctx->noSecondSet)
         for (nfcgpu_ctx::DevBuf &b: ctx->otherSet)
         {
            if (b.ptr)
               (void)hipFree(b.ptr);
            b.ptr = nullptr;
            b.bytes = 0;
         }

      if (settled)
         return settled;
      if (rc != NFCGPU_ENOMEM)
         return rc;
      ctx->lastError.clear();
   }

   return NFCGPU_OK;
}

/* What the kernels of the submission are given (W.A, W.dCfg, W.counters): the current front set's buffers, the plan's sizes, and
 * the states the front starts from - the shadow states under a tail, the slots otherwise. The lanes' buffers and the planes
 * are filled in by the stages that grow them. Queues nothing. */
void fill_scan_args(nfcgpu_ctx *ctx, WindowedSubmission &W)
{
   NfcScanArgs &A = W.A;
   uint32_t *counters = W.counters = (uint32_t *)ctx->wCounters.ptr;

   std::memset(&A, 0, sizeof(A));
   A.jobs = (NfcScanJob *)ctx->wJobs.ptr;
   A.nJobs = W.nJobs;
   A.chunks = (const NfcScanChunk *)ctx->wChunks.ptr;
   A.nChunks = W.nChunks;
   A.stride = W.stride;
   A.params = W.sp;
   A.states = W.under ? (const NfcStreamState *)ctx->wShadow.ptr : ctx->dStates;
   A.points = (NfcScanPoint *)ctx->wPoints.ptr;
   A.seams = (NfcScanSeam *)ctx->wSeams.ptr;
   A.chunkEdge = (uint32_t *)ctx->wChunkEdge.ptr;
   A.tiles = (uint32_t *)ctx->wTiles.ptr;
   A.tileStats = (NfcScanTile *)ctx->wTileStats.ptr;
   A.finalLaneSlot = W.finalLaneSlot;
   A.firstWindowSlot = W.firstWindowSlot;
   A.windowCount = counters;
   A.rerunCount = counters + 1;
   A.runCount = counters + 2;
   A.runNext = counters + 3;
   A.repairs = (NfcScanChunk *)ctx->wRepairs.ptr;
   A.repairCount = counters + 7;
   A.repairsEnv = ctx->envelopeMax ? (NfcScanChunk *)ctx->wRepairsEnv.ptr : nullptr; /* (NFCGPU_ENVELOPE_KERNEL=0: one list, one kernel) */
   A.repairEnvCount = counters + 9;
   A.saveNext = counters + 8;

   W.dCfg = ctx->dConfigs + W.config;
}

/* ---- the front: on F.fs, from A.states ---- */

/* one walk of the front. `beneath`: under the pending tail, which is advanced while the front's host waits last; `redo`: walked
 * again after the comparison (the statistics have counted its samples and second walks) */
struct FrontPass
{
   hipStream_t fs;
   bool beneath, redo;
};

/* Whatever way the front is left while its stream is not the context's own: nobody reuses what it reads or writes while it runs */
struct FrontGuard
{
   hipStream_t fs;
   bool armed;
   ~FrontGuard()
   {
      if (armed)
         (void)hipStreamSynchronize(fs);
   }
};

/* the walk that writes the planes beside the rounds, on ctx->low, likewise */
struct PlanesGuard
{
   nfcgpu_ctx *ctx;
   bool running;
   ~PlanesGuard()
   {
      if (running)
         (void)hipStreamSynchronize(ctx->low); /* (whatever way the function is left: nobody reuses what the walk reads or writes while it runs) */
   }
};

/* a host wait of the front: under a pending tail the host goes on with that instead of sleeping */
int wait_front(nfcgpu_ctx *ctx, const FrontPass &F)
{
   const hipStream_t fs = F.fs;

   if (!F.beneath)
   {
      HIP_TRY(ctx, hipStreamSynchronize(fs));
      return NFCGPU_OK;
   }

   HIP_TRY(ctx, hipEventRecord(ctx->frontEvent, fs));

   for (;;)
   {
      int r = tail_advance(ctx, false);
      if (r)
         return r;
#ifdef NFCGPU_EMULATED_TEST_BUILD
      HIP_TRY(ctx, hipEventSynchronize(ctx->frontEvent)); /* (synchronous streams: the tail has been given its turn, the front's work is done) */
      break;
#else
      const hipError_t q = hipEventQuery(ctx->frontEvent);
      if (q == hipSuccess)
         break;
      if (q != hipErrorNotReady)
         return fail(ctx, NFCGPU_EHIP, "hipEventQuery(ctx->frontEvent)", q);
      if (!ctx->tail)
      {
         HIP_TRY(ctx, hipEventSynchronize(ctx->frontEvent));
         break;
      }
      std::this_thread::sleep_for(std::chrono::microseconds(20)); /* (two events to look at, milliseconds apart: no need to spin) */
#endif
   }

   return NFCGPU_OK;
}

/* (the front leaves the submission to somebody else: whatever is pending is completed first, and the front's stream is idle - callers are behind a wait) */
int hand_over(nfcgpu_ctx *ctx, const FrontPass &F)
{
   if (F.beneath)
   {
      (void)hipStreamSynchronize(F.fs);
      return settle_tail(ctx);
   }
   return NFCGPU_OK;
}

/* the front cannot get a buffer: handed over, then the fallbacks of without_the_memory. Writes W.routed. */
int front_no_memory(nfcgpu_ctx *ctx, WindowedSubmission &W, const FrontPass &F, int code)
{
   const int handed = hand_over(ctx, F);
   W.routed = true;
   return handed ? handed : without_the_memory(ctx, W, code);
}

/* a few long busy streams (front_seam_round): handed over, then block by block. Writes W.routed. */
int front_in_blocks(nfcgpu_ctx *ctx, WindowedSubmission &W, const FrontPass &F)
{
   const int handed = hand_over(ctx, F);
   W.routed = true;
   return handed ? handed : run_in_blocks(ctx, W.config, W.items, W.stride);
}

/* Upload and first scan. Reads W.jobs and W.chunks (host) and the samples; writes the job and chunk tables, the counters and every
 * record of the scan in the current front set, and resets A.planes / A.planesStale (a second front starts as the first did). All
 * on F.fs, which under a tail first waits for the pending submission's first pass. Counts scan_samples unless `redo`. */
int front_scan(nfcgpu_ctx *ctx, WindowedSubmission &W, const FrontPass &F)
{
   const hipStream_t fs = F.fs;
   const bool beneath = F.beneath, redo = F.redo;
   NfcScanArgs &A = W.A;
   const std::vector<NfcScanJob> &jobs = W.jobs;
   const std::vector<NfcScanChunk> &chunks = W.chunks;
   const uint32_t nJobs = W.nJobs, nChunks = W.nChunks, tilesGridY = W.tilesGridY, tilesMost = W.tilesMost;
   const uint64_t totalSamples = W.totalSamples;
   const NfcConfig *dCfg = W.dCfg;
   uint32_t *counters = W.counters;

   A.planes = nullptr;
   A.planesStale = nullptr;

   HIP_TRY(ctx, hipMemcpyAsync(ctx->wJobs.ptr, jobs.data(), sizeof(NfcScanJob) * nJobs, hipMemcpyHostToDevice, fs));
   HIP_TRY(ctx, hipMemcpyAsync(ctx->wChunks.ptr, chunks.data(), sizeof(NfcScanChunk) * nChunks, hipMemcpyHostToDevice, fs));
   HIP_TRY(ctx, hipMemsetAsync(counters, 0, 256, fs));

   /* under the tail: not before the pending submission's first pass is over (the event its chain state waits for) - that pass has
    * the device to itself -, which is also behind the shadow states this front starts from */
   if (beneath && ctx->tail)
      HIP_TRY(ctx, hipStreamWaitEvent(fs, ctx->tail->ready, 0));

   mark_stage(ctx, W, "tables");

   /* scan */
   ProfiledLaunch pl {nullptr, nullptr};
   record_span(ctx, ctx->timedScan, pl, true, fs);
   hipLaunchKernelGGL(NFC_BY_LAYOUT(A.stride, nfc_scan_kernel), dim3((nChunks + NFC_LANES - 1) / NFC_LANES), dim3(NFC_LANES), 0, fs, dCfg, A);
   HIP_TRY(ctx, hipGetLastError());
   record_span(ctx, ctx->timedScan, pl, false, fs);
   if (!redo)
      ctx->stats.scan_samples += totalSamples;

   mark_stage(ctx, W, "scan");

   /* a first run of the tile tests: how busy is each stream? Only a small submission is routed by that (below: `small`); a large
    * one gets its tile flags once, when the envelopes they are formed from are the true ones (3.8 ms for the 67 M tiles of config 5) */
   if (nJobs < NFC_LANES && !ctx->inBlocks)
   {
      hipLaunchKernelGGL(nfc_tiles_kernel, dim3(nJobs, tilesGridY), dim3(256), 0, fs, dCfg, A, tilesMost);
      HIP_TRY(ctx, hipGetLastError());
   }

   return NFCGPU_OK;
}

/* Room for a planes walk beside the rounds (grow_planes) and its marks cleared, on F.fs. Without the memory the submission is
 * routed (front_no_memory). */
int front_beside_room(nfcgpu_ctx *ctx, WindowedSubmission &W, const FrontPass &F)
{
   const hipStream_t fs = F.fs;
   const uint32_t nChunks = W.nChunks;
   int rc;

   if ((rc = grow_planes(ctx, W, nChunks, true)))
      return front_no_memory(ctx, W, F, rc);

   HIP_TRY(ctx, hipMemsetAsync(ctx->wPlanesStale.ptr, 0, 4u * (size_t)nChunks, fs));
   return NFCGPU_OK;
}

/* NFCGPU_WINDOW_DEBUG=4: which fields keep seams from verifying (host-side look at the records the seam check is about to judge).
 * Waits for the front and copies the seam records back; changes nothing. */
int dump_seams(nfcgpu_ctx *ctx, WindowedSubmission &W, const FrontPass &F, uint32_t round)
{
   const std::vector<NfcScanJob> &jobs = W.jobs;
   const uint32_t nJobs = W.nJobs, nChunks = W.nChunks;
   int rc;

   std::vector<NfcScanSeam> sm(nChunks);
   if ((rc = wait_front(ctx, F)))
      return rc;
   HIP_TRY(ctx, hipMemcpy(sm.data(), ctx->wSeams.ptr, sizeof(NfcScanSeam) * nChunks, hipMemcpyDeviceToHost));
   uint32_t n[8] = {0, 0, 0, 0, 0, 0, 0, 0};
   for (uint32_t j = 0; j < nJobs; j++)
      for (uint32_t k = 1; k < jobs[j].chunks; k++)
      {
         const NfcScanPoint &a = sm[jobs[j].firstChunk + k].start, &b = sm[jobs[j].firstChunk + k - 1].end;
         const bool env = std::memcmp(&a.env, &b.env, 4) != 0 || a.pulseFilter != b.pulseFilter;
         const bool n1 = std::memcmp(&a.n1, &b.n1, 4) != 0, mdev = std::memcmp(&a.mdev, &b.mdev, 4) != 0, avg = std::memcmp(&a.avg, &b.avg, 4) != 0;
         const bool peak = std::memcmp(&a.edgePeak, &b.edgePeak, 4) != 0, zone = ((a.zone ^ b.zone) & 0xFFu) != 0;
         const bool time = (a.zone & 0x100u) && (b.zone & 0x100u) && a.edgeTime != b.edgeTime;
         n[0] += env; n[1] += n1; n[2] += mdev; n[3] += avg; n[4] += peak; n[5] += zone; n[6] += time;
         n[7] += (n1 || mdev || avg || peak || zone) ? 1u : 0u;
      }
   std::fprintf(stderr, "[nfcgpu]    before round %u, seams that differ in: envelope / counter %u, n1 %u, deviation %u, average %u, edge peak %u, zone %u, known edge times %u; in anything but the envelope %u\n",
                round, n[0], n[1], n[2], n[3], n[4], n[5], n[6], n[7]);
   return NFCGPU_OK;
}

/* One seam round on F.fs: the seam check, its counts to the host (a host wait), and the second walks of the chunks it listed -
 * the scan kernel, the envelope kernel or both. *found: the chunks walked again; none ends the rounds. Round 0 of a small
 * submission also reads the job table back into W.jobs (the tile tests have counted its busy tiles) and may route the submission
 * to blocks (W.routed). Reads and rewrites the seam and point records of the current front set; counts scan_repairs unless `redo`. */
int front_seam_round(nfcgpu_ctx *ctx, WindowedSubmission &W, const FrontPass &F, uint32_t round, uint32_t *found)
{
   const hipStream_t fs = F.fs;
   const bool redo = F.redo;
   const NfcScanArgs &A = W.A;
   std::vector<NfcScanJob> &jobs = W.jobs;
   const uint32_t nJobs = W.nJobs;
   const bool debugStages = W.debugStages;
   const NfcConfig *dCfg = W.dCfg;
   uint32_t *counters = W.counters;
   int rc;

   HIP_TRY(ctx, hipMemsetAsync(counters + 7, 0, 4, fs));
   HIP_TRY(ctx, hipMemsetAsync(counters + 9, 0, 4, fs));
   hipLaunchKernelGGL(nfc_seams_kernel, dim3((nJobs + 63) / 64), dim3(64), 0, fs, A, round == 0 ? 1u : 0u);
   HIP_TRY(ctx, hipGetLastError());

   /* chunks to walk again: every recurrence of them (A.repairs), the envelope tracker alone (A.repairsEnv: listed apart by
    * the seam check when the envelope kernel is on) */
   uint32_t *word = ctx->frontHost; /* (pinned: the copy does not hold the host, which has a tail to advance) */
   HIP_TRY(ctx, hipMemcpyAsync(word, counters + 7, 12, hipMemcpyDeviceToHost, fs));

   /* (a small submission: how busy are its streams? the tile tests have counted) */
   const bool small = round == 0 && nJobs < NFC_LANES && !ctx->inBlocks;
   if (small)
      HIP_TRY(ctx, hipMemcpyAsync(jobs.data(), ctx->wJobs.ptr, sizeof(NfcScanJob) * nJobs, hipMemcpyDeviceToHost, fs));

   if ((rc = wait_front(ctx, F)))
      return rc;
   const uint32_t whole = word[0], alone = word[2];
   const uint32_t repairs = *found = whole + alone;

   /* A few long busy streams: the passes the chain needs grow with the length of the submission (a frame that changes
    * the protocol timing is learnt one generation per pass), so it is decoded in blocks, each settled before the next.
    * Nothing has been touched yet (the scan only reads). */
   if (small)
   {
      uint32_t longest = 0;
      bool busy = false;

      for (uint32_t j = 0; j < nJobs; j++)
      {
         const uint64_t nTiles = ((uint64_t)jobs[j].count + NFC_SCAN_TILE - 1) / NFC_SCAN_TILE;
         busy = busy || (uint64_t)jobs[j].busyTiles * 100u > nTiles * ctx->busyPercent;
         longest = jobs[j].count > longest ? jobs[j].count : longest;
      }

      if (busy && longest > ctx->blockSamples)
         return front_in_blocks(ctx, W, F);
   }

   if (debugStages)
      std::fprintf(stderr, "[nfcgpu]    seams round %u: %u chunks to walk again\n", round, repairs);

   if (!repairs)
      return NFCGPU_OK;

   /* The chunks whose envelope tracker alone started wrong - from the second round on that is all of them: chains of chunks
    * that inherit a wrong envelope from each other, a chunk per round - go to a kernel that does nothing else, a wavefront
    * per chunk (nfc_envelope.hpp): a round then costs the tracker's own latency over one chunk instead of the scan kernel's
    * row machinery over it (9 ms of 32768 samples, however short the list). A list too long for a wave a chunk to pay (the
    * first round of a large submission: a quarter of its chunks, the scan kernel's 64 chunks per wave are the better use
    * of the machine) stays with the scan kernel's envelope-only branch (NFCGPU_ENVELOPE_KERNEL: the longest list the
    * envelope kernel is given). */
   if (debugStages && alone && alone <= ctx->envelopeMax)
      std::fprintf(stderr, "[nfcgpu]    ... %u of them the envelope tracker's alone, by the envelope kernel\n", alone);

   ProfiledLaunch pr {nullptr, nullptr};
   record_span(ctx, ctx->timedScan, pr, true, fs);

   const bool byWaves = alone && alone <= ctx->envelopeMax;

   if (whole || (alone && !byWaves))
   {
      /* the scan kernel: the chunks walked whole, and a list of envelope-only ones too long for a wave each, in one launch */
      NfcScanArgs R = A;
      R.chunks = A.repairs;
      R.nChunks = whole;
      R.chunksMore = byWaves ? nullptr : A.repairsEnv;
      R.nChunksMore = byWaves ? 0u : alone;

      const uint32_t listedNow = R.nChunks + R.nChunksMore;

      hipLaunchKernelGGL(NFC_BY_LAYOUT(R.stride, nfc_scan_kernel), dim3((listedNow + NFC_LANES - 1) / NFC_LANES), dim3(NFC_LANES), 0, fs, dCfg, R);
      HIP_TRY(ctx, hipGetLastError());
   }

   if (byWaves)
   {
      NfcScanArgs R = A;
      R.chunks = A.repairsEnv;
      R.nChunks = alone;
      R.followChains = alone <= ctx->envelopeFollowMax ? 1u : 0u;

      hipLaunchKernelGGL(NFC_BY_LAYOUT(R.stride, nfc_envelope_kernel), dim3(alone), dim3(NFC_LANES), 0, fs, dCfg, R);
      HIP_TRY(ctx, hipGetLastError());
   }

   record_span(ctx, ctx->timedScan, pr, false, fs);
   if (!redo)
      ctx->stats.scan_repairs += repairs;

   return NFCGPU_OK;
}

/* The planes of every chunk, beside the rounds to come: on ctx->low, behind what F.fs has queued so far (planesFork); planesJoin is
 * recorded behind the walk and `planesGuard` armed. From here on the rounds note the start states they rewrite (A.planesStale).
 * Reads the points the first round has left; writes ctx->wPlanes. */
int front_planes_beside(nfcgpu_ctx *ctx, WindowedSubmission &W, const FrontPass &F, PlanesGuard &planesGuard)
{
   const hipStream_t fs = F.fs;
   NfcScanArgs &A = W.A;
   const NfcScanParams &sp = W.sp;
   const uint32_t nChunks = W.nChunks;
   const NfcConfig *dCfg = W.dCfg;

   HIP_TRY(ctx, hipEventRecord(ctx->planesFork, fs));
   HIP_TRY(ctx, hipStreamWaitEvent(ctx->low, ctx->planesFork, 0));
   planesGuard.running = true;

   NfcScanArgs P = A;
   P.planes = (float *)ctx->wPlanes.ptr;
   P.chunks = (const NfcScanChunk *)ctx->wChunks.ptr; /* (the submission's chunk table as it is: the walk takes no notice of the repair marks) */
   P.nChunks = nChunks;
   /* a lane per piece, and the pieces of a chunk have to tile it: the largest multiple of the distance of the stored
    * points (every lane starts from one) that is no longer than NFCGPU_PLANES_BESIDE_PIECE and divides the chunk. (Until
    * round 6 the quotient was truncated: with a chunk that is no multiple of the piece - the default sizing gives any
    * multiple of 512 for totals between 2^28 and 2^30 samples - the tail of every chunk that was not walked again got no
    * planes at all.) A chunk is a multiple of the points' distance, so that distance always does. */
   P.planesPiece = ctx->planesBesidePiece / NFC_SCAN_POINT * NFC_SCAN_POINT;
   if (P.planesPiece > sp.chunkSamples)
      P.planesPiece = sp.chunkSamples / NFC_SCAN_POINT * NFC_SCAN_POINT;
   while (P.planesPiece > NFC_SCAN_POINT && sp.chunkSamples % P.planesPiece != 0u)
      P.planesPiece -= NFC_SCAN_POINT;
   if (P.planesPiece && sp.chunkSamples % P.planesPiece != 0u)
      P.planesPiece = 0u; /* (a chunk that is no multiple of the points' distance: a lane per chunk, from its start) */
   P.planesPerChunk = P.planesPiece ? sp.chunkSamples / P.planesPiece : 0u;

   const uint64_t lanesOfIt = (uint64_t)nChunks * (P.planesPerChunk ? P.planesPerChunk : 1u);

   ProfiledLaunch pp {nullptr, nullptr};
   record_span(ctx, ctx->timedPlanes, pp, true, ctx->low);
   hipLaunchKernelGGL(NFC_BY_LAYOUT(P.stride, nfc_scan_planes_kernel), dim3((uint32_t)((lanesOfIt + NFC_LANES - 1) / NFC_LANES)), dim3(NFC_LANES), 0, ctx->low, dCfg, P);
   HIP_TRY(ctx, hipGetLastError());
   record_span(ctx, ctx->timedPlanes, pp, false, ctx->low);
   HIP_TRY(ctx, hipEventRecord(ctx->planesJoin, ctx->low));

   A.planesStale = (uint32_t *)ctx->wPlanesStale.ptr; /* from the next round on */
   return NFCGPU_OK;
}

/* the tile flags, from the envelopes the rounds have left true: on F.fs, into A.tiles and the jobs' counts */
int front_tile_flags(nfcgpu_ctx *ctx, WindowedSubmission &W, const FrontPass &F)
{
   const hipStream_t fs = F.fs;
   const NfcScanArgs &A = W.A;

   hipLaunchKernelGGL(nfc_tiles_kernel, dim3(W.nJobs, W.tilesGridY), dim3(256), 0, fs, W.dCfg, A, W.tilesMost);
   HIP_TRY(ctx, hipGetLastError());

   mark_stage(ctx, W, "seams");

   return NFCGPU_OK;
}

/* The planes after the rounds when their walk ran beside: F.fs waits for the walk (planesJoin; the guard is disarmed), the chunks
 * whose start state changed under it are listed into ctx->wPlaneChunks and counted (a host wait), and walked again on F.fs.
 * Sets A.planes; A.planesStale is done with. */
int front_planes_again(nfcgpu_ctx *ctx, WindowedSubmission &W, const FrontPass &F, PlanesGuard &planesGuard)
{
   const hipStream_t fs = F.fs;
   NfcScanArgs &A = W.A;
   const NfcScanParams &sp = W.sp;
   const uint32_t nChunks = W.nChunks;
   const bool debugStages = W.debugStages;
   const NfcConfig *dCfg = W.dCfg;
   uint32_t *counters = W.counters;
   int rc;

   /* the walk over all chunks has run beside the rounds: the chunks whose start state changed under it, again */
   HIP_TRY(ctx, hipStreamWaitEvent(fs, ctx->planesJoin, 0));
   planesGuard.running = false; /* (the main stream now waits for it) */

   HIP_TRY(ctx, hipMemsetAsync(counters + 11, 0, 4, fs));
   hipLaunchKernelGGL(nfc_planes_stale_kernel, dim3((nChunks + 255) / 256), dim3(256), 0, fs, A, (const NfcScanChunk *)ctx->wChunks.ptr, nChunks,
                      (NfcScanChunk *)ctx->wPlaneChunks.ptr, counters + 11);
   HIP_TRY(ctx, hipGetLastError());

   uint32_t &again = ctx->frontHost[4];
   HIP_TRY(ctx, hipMemcpyAsync(ctx->frontHost + 4, counters + 11, 4, hipMemcpyDeviceToHost, fs));
   if ((rc = wait_front(ctx, F)))
      return rc;

   A.planes = (float *)ctx->wPlanes.ptr;
   A.planesStale = nullptr;

   if (debugStages)
      std::fprintf(stderr, "[nfcgpu]    planes written beside the rounds; %u chunks of %u again\n", again, nChunks);

   if (again)
   {
      NfcScanArgs P = A;
      /* (a stored point per lane - 512 samples, from the points the rounds have left true -: a few thousand chunks a lane each
       * would take as long as one chunk's walk, 12 ms, with the device all but idle) */
      P.chunks = (const NfcScanChunk *)ctx->wPlaneChunks.ptr;
      P.nChunks = again;
      P.planesPiece = NFC_SCAN_POINT;
      P.planesPerChunk = sp.chunkSamples / NFC_SCAN_POINT;

      ProfiledLaunch pp {nullptr, nullptr};
      record_span(ctx, ctx->timedPlanes, pp, true, fs);
      hipLaunchKernelGGL(NFC_BY_LAYOUT(P.stride, nfc_scan_planes_kernel), dim3((uint32_t)(((uint64_t)again * P.planesPerChunk + NFC_LANES - 1) / NFC_LANES)), dim3(NFC_LANES), 0, fs, dCfg, P);
      HIP_TRY(ctx, hipGetLastError());
      record_span(ctx, ctx->timedPlanes, pp, false, fs);
   }

   mark_stage(ctx, W, "planes");

   return NFCGPU_OK;
}

/* The planes after the rounds when no walk ran beside them: every chunk - of a small submission every piece - is listed on the
 * host, uploaded and walked on F.fs, which is then waited for: the list is a local. Grows the planes' buffers (without the memory
 * the submission is routed: front_no_memory) and sets A.planes. Reads W.jobs and W.chunks. */
int front_planes_after(nfcgpu_ctx *ctx, WindowedSubmission &W, const FrontPass &F)
{
   const hipStream_t fs = F.fs;
   NfcScanArgs &A = W.A;
   const std::vector<NfcScanJob> &jobs = W.jobs;
   const std::vector<NfcScanChunk> &chunks = W.chunks;
   const uint32_t nJobs = W.nJobs;
   const uint64_t totalSamples = W.totalSamples;
   const NfcConfig *dCfg = W.dCfg;
   int rc;

   /* A small submission - one a caller waits for - is walked a lane per stored point instead of a lane per chunk: 512 samples
    * instead of 4096 on the way of everything that follows (NFCGPU_PLANES_PIECE; a short capture: 1.1 -> 0.2 ms) */
   const uint32_t piece = totalSamples <= (4u << 20) ? ctx->planesPiece / NFC_SCAN_POINT * NFC_SCAN_POINT : 0u;

   std::vector<NfcScanChunk> all;

   if (piece)
   {
      for (uint32_t j = 0; j < nJobs; j++)
         for (uint32_t i = 0; i * piece < jobs[j].count; i++)
            all.push_back(NfcScanChunk {j, i | NFC_CHUNK_REPAIR});
   }
   else
   {
      all = chunks;
      for (NfcScanChunk &c: all)
         c.index |= NFC_CHUNK_REPAIR;
   }

   const uint32_t nPlaneLanes = (uint32_t)all.size();

   if ((rc = grow_planes(ctx, W, all.size(), false)))
      return front_no_memory(ctx, W, F, rc);

   HIP_TRY(ctx, hipMemcpyAsync(ctx->wPlaneChunks.ptr, all.data(), sizeof(NfcScanChunk) * all.size(), hipMemcpyHostToDevice, fs));

   A.planes = (float *)ctx->wPlanes.ptr;

   NfcScanArgs P = A;
   P.chunks = (const NfcScanChunk *)ctx->wPlaneChunks.ptr;
   P.nChunks = nPlaneLanes;
   P.planesPiece = piece;

   ProfiledLaunch pp {nullptr, nullptr};
   record_span(ctx, ctx->timedPlanes, pp, true, fs);
   hipLaunchKernelGGL(NFC_BY_LAYOUT(P.stride, nfc_scan_planes_kernel), dim3((nPlaneLanes + NFC_LANES - 1) / NFC_LANES), dim3(NFC_LANES), 0, fs, dCfg, P);
   HIP_TRY(ctx, hipGetLastError());
   record_span(ctx, ctx->timedPlanes, pp, false, fs);
   if ((rc = wait_front(ctx, F)))
      return rc; /* (the chunk list is a local) */

   mark_stage(ctx, W, "planes");

   return NFCGPU_OK;
}

/* The front of a submission: upload and scan, seam rounds until every chunk starts from the true state, the tile flags, the
 * planes. Everything on F.fs but a planes walk beside the rounds (ctx->low); left early - an error, a submission routed
 * elsewhere - the streams it used are waited for by the guards. */
int front(nfcgpu_ctx *ctx, WindowedSubmission &W, const FrontPass &F)
{
   FrontGuard frontGuard {F.fs, F.beneath};
   int rc;

   if ((rc = front_scan(ctx, W, F)))
      return rc;

   /* The front-end planes (below) are a walk of every chunk from its verified start state: 69 GB of stores for config 5, 32 ms
    * of a device that the rounds of second walks after the first leave nearly idle (a few thousand chunks each, as long as
    * their longest chain). Round 5: for a large submission that walk is started on a stream of its own (lowest priority) as soon as the first round's
    * second walks are queued - by then nine chunks in ten start from their true state -, the seam check and the envelope
    * walks note every start state they rewrite from then on (NfcScanArgs::planesStale), and those chunks' planes are written
    * again when the rounds are over. */
   const bool planesBeside = ctx->planesBeside && ctx->low != nullptr && W.totalSamples > (4u << 20);
   bool planesStarted = false;
   PlanesGuard planesGuard {ctx, false};

   if (planesBeside && ((rc = front_beside_room(ctx, W, F)) || W.routed))
      return rc;

   /* seams: chunks that did not start from the true state are walked again, a round at a time */
   for (uint32_t round = 0;; round++)
   {
      uint32_t repairs = 0;

      if (W.debugStages && W.debugLevel >= 4 && (rc = dump_seams(ctx, W, F, round)))
         return rc;

      if ((rc = front_seam_round(ctx, W, F, round, &repairs)) || W.routed)
         return rc;

      if (!repairs)
         break;

      if (planesBeside && round == 0)
      {
         if ((rc = front_planes_beside(ctx, W, F, planesGuard)))
            return rc;
         planesStarted = true;
      }
   }

   if ((rc = front_tile_flags(ctx, W, F)))
      return rc;

   /* The wave decoder takes the front end's results per sample instead of walking it again: a second walk of every
    * chunk from its verified start state (the repair form of the scan: no warm-up) writes them. */
   rc = planesStarted ? front_planes_again(ctx, W, F, planesGuard) : front_planes_after(ctx, W, F);
   if (rc || W.routed)
      return rc;

   frontGuard.armed = false;
   return NFCGPU_OK;
}

/* The join of a front that ran under the pending tail: the tail is completed, the context's stream takes the front's work in
 * (frontEvent), and the shadow states the front started from are compared with what the finish really left (a host wait on
 * ctx->stream). The same but for zeroed edge times: the records are put right on ctx->stream. Anything else: the front again,
 * on ctx->stream, from the slots (A.states). Counts pipelined_submissions, pipeline_zeroed_edges, pipeline_refronts. */
int join_front(nfcgpu_ctx *ctx, WindowedSubmission &W)
{
   NfcScanArgs &A = W.A;
   const uint32_t nJobs = W.nJobs;
   int rc;

   ctx->stats.pipelined_submissions++;

   /* the tail, finish and any sequential fallback of its invalid jobs included; then the main stream takes the front's work in */
   if ((rc = settle_tail(ctx)))
   {
      (void)hipStreamSynchronize(ctx->front);
      return rc;
   }

   HIP_TRY(ctx, hipEventRecord(ctx->frontEvent, ctx->front));
   HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->frontEvent, 0));

   /* exact or not taken: what the finish really left in the slots against the shadow states the front started from */
   NfcShadowArgs S;
   std::memset(&S, 0, sizeof(S));
   S.jobs = A.jobs;
   S.nJobs = nJobs;
   S.real = ctx->dStates;
   S.shadow = (NfcStreamState *)ctx->wShadow.ptr;
   S.ctl = (uint32_t *)ctx->wShadowCtl.ptr;

   S.points = A.points;
   S.renameSeams = A.seams;
   S.renameEdge = A.chunkEdge;

   HIP_TRY(ctx, hipMemsetAsync(S.ctl, 0, 64, ctx->stream));
   hipLaunchKernelGGL(nfc_shadow_compare_kernel, dim3((nJobs + 63) / 64), dim3(64), 0, ctx->stream, S);
   HIP_TRY(ctx, hipGetLastError());
   HIP_TRY(ctx, hipMemcpyAsync(ctx->tailHost + 16, S.ctl, 64, hipMemcpyDeviceToHost, ctx->stream));
   HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));

   const uint32_t differ = ctx->tailHost[16], zeroed = ctx->tailHost[26];
   A.states = ctx->dStates;

   if (ctx->pipelineReport && !differ)
      std::fprintf(stderr, "[nfcgpu] pipelined front: %u streams ended on a zeroed edge time (put right in the records), none differs otherwise\n", zeroed);

   if (!differ)
      ctx->stats.pipeline_zeroed_edges += zeroed;

   if (zeroed && !differ)
   {
      /* (a carrier frame after the tracker last moved: NfcShadowArgs) */
      hipLaunchKernelGGL(nfc_shadow_rename_kernel, dim3(nJobs), dim3(64), 0, ctx->stream, S);
      HIP_TRY(ctx, hipGetLastError());
   }

   if (differ)
   {
      /* streams that did not end where their front-end records said (a stream the sequential kernels decoded, say): the front
       * again, unpipelined, from the true state */
      const uint32_t *f = ctx->tailHost + 16;
      ctx->stats.pipeline_refronts += differ;

      if (ctx->pipelineReport)
         std::fprintf(stderr, "[nfcgpu] pipelined front redone: %u streams differ from their shadow state otherwise than by a zeroed edge time (clock %u, pulse counter %u, envelope %u, n1 %u, deviation %u, average %u, "
                              "edge peak %u, edge time %u, carrier zone %u)\n", f[0], f[1], f[2], f[3], f[4], f[5], f[6], f[7], f[8], f[9]);

      return front(ctx, W, FrontPass {ctx->stream, false, true});
   }

   return NFCGPU_OK;
}

/* ---- the back: on the context's stream, the streams' own slots ---- */

/* records per lane slot (carry lanes, final lanes, one per window); ring and frame-assembly storage per carry lane,
 * final lane and per lane of the persistent waves that run the windows */
int grow_lanes(nfcgpu_ctx *ctx, const WindowedSubmission &W, uint32_t lanesWanted)
{
   const size_t storageLanes = (size_t)W.firstWindowSlot; /* (a speculative window's rings live in LDS; one that runs to the end leaves a copy in the save area) */
   const size_t lanes = ((size_t)lanesWanted + NFC_LANES - 1) / NFC_LANES * NFC_LANES;
   int r;
   if ((r = grow(ctx, ctx->wWindows, sizeof(NfcWindow) * lanes)) || (r = grow(ctx, ctx->wWorks, sizeof(NfcWork) * lanes)) ||
       (r = grow(ctx, ctx->vStates, sizeof(NfcStreamState) * lanes)) || (r = grow(ctx, ctx->vCold, sizeof(NfcStreamCold) * lanes)) ||
       (r = grow(ctx, ctx->wRunList, 4 * lanes)) ||
       (r = grow(ctx, ctx->vRings, sizeof(float) * (size_t)kRingBlockFloats * (storageLanes / NFC_LANES))) ||
       (r = grow(ctx, ctx->vBytes, (size_t)NFC_STREAM_BYTES * storageLanes)))
      return r;
   return NFCGPU_OK;
}

/* The lane buffers: room for a first guess at the windows, or what an earlier, larger submission has left. Sets A.windows, A.works,
 * A.runList and A.windowRoom; without the memory the submission is routed. Queues nothing. */
int back_lane_buffers(nfcgpu_ctx *ctx, WindowedSubmission &W)
{
   NfcScanArgs &A = W.A;
   const uint32_t nJobs = W.nJobs, firstWindowSlot = W.firstWindowSlot;
   const uint64_t totalSamples = W.totalSamples;
   int rc;

   /* lanes: a first guess (one window per 8192 samples); the window kernel reports what it needs */
   uint32_t room = (uint32_t)(totalSamples / 8192) + 2 * nJobs + 64;

   /* is there room already from an earlier, larger submission? */
   {
      /* (every lane buffer has to hold them: one that could not be grown last time - NFCGPU_ENOMEM, the submission then taken in
       * quarters - must not be asked for the room its neighbours got) */
      size_t have = ctx->wWindows.bytes / sizeof(NfcWindow);
      have = std::min(have, ctx->wWorks.bytes / sizeof(NfcWork));
      have = std::min(have, ctx->vStates.bytes / sizeof(NfcStreamState));
      have = std::min(have, ctx->vCold.bytes / sizeof(NfcStreamCold));
      have = std::min(have, ctx->wRunList.bytes / 4);
      if (have > (size_t)firstWindowSlot + room)
         room = (uint32_t)(have - firstWindowSlot - NFC_LANES);
   }

   if ((rc = grow_lanes(ctx, W, firstWindowSlot + room)))
      return without_the_memory(ctx, W, rc);

   A.windows = (NfcWindow *)ctx->wWindows.ptr;
   A.works = (NfcWork *)ctx->wWorks.ptr;
   A.windowRoom = room;
   A.runList = (uint32_t *)ctx->wRunList.ptr;
   return NFCGPU_OK;
}

/* The staging sink of the lanes' frame records, its control words cleared on ctx->stream, and the save area of lanes that run to
 * the end of the submission (A.saveRings, A.saveBytes, A.saveRoom). Without the memory the submission is routed. */
int back_sink_and_save(nfcgpu_ctx *ctx, WindowedSubmission &W)
{
   NfcScanArgs &A = W.A;
   const uint32_t nJobs = W.nJobs;
   int rc;

   /* staging sink for the lanes' chained frame records (lanes that turn out not to be live write theirs too): room
    * for four times the frame sink, at least 64 MiB; what does not fit is reported as dropped like any overflow */
   {
      size_t staging = (size_t)ctx->ownSinkWords * 16;
      if (staging < (64u << 20))
         staging = 64u << 20;
      if (staging > 0xFFFFFFF0ull * 4ull)
         staging = 0xFFFFFFF0ull * 4ull;
      if ((rc = grow(ctx, ctx->vSink, staging)) || (rc = grow(ctx, ctx->vSinkCtl, 16)))
         return without_the_memory(ctx, W, rc);
   }

   HIP_TRY(ctx, hipMemsetAsync(ctx->vSinkCtl.ptr, 0, 16, ctx->stream));

   /* save area for lanes that run to the end of the submission (nfc_scan_launch.h): a few per stream */
   {
      const uint32_t saveRoom = 2 * nJobs + 1024;
      if ((rc = grow(ctx, ctx->vSaveRings, sizeof(float) * (size_t)(kRingBlockFloats / NFC_LANES) * saveRoom)) ||
          (rc = grow(ctx, ctx->vSaveBytes, (size_t)NFC_STREAM_BYTES * saveRoom)))
         return without_the_memory(ctx, W, rc);

      A.saveRings = (float *)ctx->vSaveRings.ptr;
      A.saveBytes = (uint8_t *)ctx->vSaveBytes.ptr;
      A.saveRoom = saveRoom;
   }

   return NFCGPU_OK;
}

/* The shadow states a submission that continues these streams may start its front from while this one's tail is pending: the
 * slot as the front found it, its front-end fields set from the end of the last chunk - the front end is a function of the
 * samples, and once the rounds are over that end is the true one - the way nfc_window_lane turns a point into state. (Nobody
 * reads the shadows of the submission before any more: its successor's front - this one - has been joined.)
 *
 * Sets W.shadows; the first time grows ctx->wShadow / wShadowCtl (a device that cannot give them: noSecondSet). The kernel runs on
 * ctx->stream and reads the slots and the seam records. */
int back_shadow_states(nfcgpu_ctx *ctx, WindowedSubmission &W)
{
   const NfcScanArgs &A = W.A;
   const uint32_t nJobs = W.nJobs;
   const bool shadows = W.shadows = ctx->pipeline && !ctx->inBlocks && !W.debugStages && ctx->deferOK && !ctx->noSecondSet && ctx->front != nullptr;

   if (shadows && !ctx->wShadow.ptr)
   {
      if (grow(ctx, ctx->wShadow, sizeof(NfcStreamState) * (size_t)ctx->maxStreams) || grow(ctx, ctx->wShadowCtl, 64 + 4 * (size_t)ctx->maxStreams))
      {
         (void)hipGetLastError();
         ctx->noSecondSet = true;
         ctx->lastError.clear();
      }
   }

   if (shadows && ctx->wShadow.ptr && ctx->wShadowCtl.ptr)
   {
      NfcShadowArgs S;
      std::memset(&S, 0, sizeof(S));
      S.jobs = A.jobs;
      S.nJobs = nJobs;
      S.seams = A.seams;
      S.chunkEdge = A.chunkEdge;
      S.from = ctx->dStates; /* (whatever was pending has been completed: the slots are what this submission starts from) */
      S.shadow = (NfcStreamState *)ctx->wShadow.ptr;
      S.spoil = ctx->spoilShadow;

      hipLaunchKernelGGL(nfc_shadow_kernel, dim3((nJobs + 63) / 64), dim3(64), 0, ctx->stream, S);
      HIP_TRY(ctx, hipGetLastError());
   }

   return NFCGPU_OK;
}

/* Window placement on ctx->stream, a host wait for the count (W.nWindows); again with more room when the guess was short. May
 * grow the lane buffers and set A's pointers to them anew; without the memory the submission is routed. */
int back_place_windows(nfcgpu_ctx *ctx, WindowedSubmission &W)
{
   NfcScanArgs &A = W.A;
   const uint32_t nJobs = W.nJobs, firstWindowSlot = W.firstWindowSlot;
   uint32_t *counters = W.counters;
   uint32_t &nWindows = W.nWindows;
   uint32_t room = A.windowRoom;
   int rc;

   for (int attempt = 0; attempt < 2; attempt++)
   {
      hipLaunchKernelGGL(nfc_windows_kernel, dim3(nJobs), dim3(64), 0, ctx->stream, A);
      HIP_TRY(ctx, hipGetLastError());
      HIP_TRY(ctx, hipMemcpyAsync(&nWindows, counters, 4, hipMemcpyDeviceToHost, ctx->stream));
      HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));

      if (nWindows <= room)
         break;

      room = nWindows + NFC_LANES;
      if ((rc = grow_lanes(ctx, W, firstWindowSlot + room)))
         return without_the_memory(ctx, W, rc);

      A.windows = (NfcWindow *)ctx->wWindows.ptr;
      A.works = (NfcWork *)ctx->wWorks.ptr;
      A.runList = (uint32_t *)ctx->wRunList.ptr;
      A.windowRoom = room;
      HIP_TRY(ctx, hipMemsetAsync(counters, 0, 4, ctx->stream));
   }

   mark_stage(ctx, W, "windows");

   return NFCGPU_OK;
}

/* The lanes' launch record, the carry lanes on ctx->stream and the hand-off: a WindowedTail takes what is left of the submission,
 * is advanced to the end of the first pass and the chain kernel behind it (host waits) and then either stays pending on the
 * context - the rule is below - or is completed here. */
int back_lanes_and_tail(nfcgpu_ctx *ctx, WindowedSubmission &W)
{
   const NfcScanArgs &A = W.A;
   const uint32_t nJobs = W.nJobs, nWindows = W.nWindows;
   uint32_t *counters = W.counters;
   const bool shadows = W.shadows;
   int rc;

   NfcLaunch real = base_launch(ctx);

   NfcLaunch lanes;
   std::memset(&lanes, 0, sizeof(lanes));
   lanes.states = (NfcStreamState *)ctx->vStates.ptr;
   lanes.cold = (NfcStreamCold *)ctx->vCold.ptr;
   lanes.rings = (float *)ctx->vRings.ptr;
   lanes.bytes = (uint8_t *)ctx->vBytes.ptr;
   lanes.sink = (uint32_t *)ctx->vSink.ptr;
   lanes.sinkCtl = (uint32_t *)ctx->vSinkCtl.ptr;
   lanes.sinkWords = (uint32_t)(ctx->vSink.bytes / 4 > 0xFFFFFFF0ull ? 0xFFFFFFF0ull : ctx->vSink.bytes / 4);
   if (ctx->stagingWords && lanes.sinkWords > ctx->stagingWords)
      lanes.sinkWords = ctx->stagingWords; /* (NFCGPU_STAGING_WORDS: the tests make it run full) */
   lanes.ringBlockFloats = kRingBlockFloats;
   lanes.works = (const NfcWork *)ctx->wWorks.ptr;
   lanes.windows = (NfcWindow *)ctx->wWindows.ptr;
   lanes.jobs = (const NfcScanJob *)ctx->wJobs.ptr;
   lanes.laneStats = counters + 4;
   lanes.uniformStride = W.stride;

   /* lanes */
   hipLaunchKernelGGL(nfc_carry_lanes_kernel, dim3(nJobs), dim3(NFC_LANES), 0, ctx->stream, A, real, lanes, 0u);
   HIP_TRY(ctx, hipGetLastError());

   const uint32_t windowBlocks = (nWindows + NFC_LANES - 1) / NFC_LANES;

   WindowedTail *T = new (std::nothrow) WindowedTail();
   if (!T)
      return fail(ctx, NFCGPU_ENOMEM, "out of host memory");

   T->config = W.config;
   T->stride = W.stride;
   T->items = W.items;
   T->A = A;
   T->real = real;
   T->lanes = lanes;
   T->dCfg = W.dCfg;
   T->counters = counters;
   T->dJobs = ctx->wJobs.ptr;
   T->nJobs = nJobs;
   T->nWindows = nWindows;
   T->windowBlocks = windowBlocks;
   T->firstWindowSlot = W.firstWindowSlot;
   T->finalLaneSlot = W.finalLaneSlot;
   T->totalSamples = W.totalSamples;
   T->debugStages = W.debugStages;
   T->stageBegan = W.stageBegan;
   T->ready = take_event(ctx);
   record_span(ctx, ctx->timedWindow, T->pw, true);

   ctx->tail = T;

   if ((rc = tail_list(ctx, *T)))
   {
      ctx->tail = nullptr;
      ctx->eventPool.push_back(T->ready);
      delete T;
      return rc;
   }

   /* the first pass and the chain kernel behind it */
   while (ctx->tail && !(T->state == WindowedTail::Chain && T->pass == 0))
      if ((rc = tail_advance(ctx, true)))
         return rc;

   /* The rest may stay pending for the next submission to run its front under (one that continues these streams; anything else
    * completes it first) - not when the call has to have the device's answer: a block of run_in_blocks, a stage log, a caller
    * that did not come through nfcgpu_submit_uniform. */
   if (ctx->tail && shadows && ctx->wShadow.ptr && ctx->wShadowCtl.ptr && !std::getenv("NFCGPU_WAVE_VERIFY_REPORT") && !ctx->dumpWindows)
   {
      T->deferred = true;
      return NFCGPU_OK;
   }

   return settle_tail(ctx);
}

/* One submission of `items` (all of configuration `config`, `stride` floats per sample, data resident on the device)
 * through scan -> windows -> windowed decode -> chain -> finish; streams the path cannot vouch for (samples off the
 * int16 grid, a seam that did not verify, no settled chain) are then decoded sequentially from their untouched state.
 *
 * It has a front - tables, scan, seam rounds, planes, tile flags: a function of the samples and of the front-end state the
 * streams start from - and a back: windows, decode passes, chain, finish. The back's own end (WindowedTail) may stay pending
 * when the call returns; a submission that continues the same streams then runs its front under it, on ctx->front, from the
 * shadow states the pending submission's back has left for it (nfc_shadow_kernel), and once the tail is done has the shadows
 * compared with what the finish really wrote: a front that started from anything else is walked again from the true state.
 *
 * In the order of the stages above: plan, buffers, front - or front under the tail, then the join -, back, tail. */
int run_windowed(nfcgpu_ctx *ctx, uint32_t config, const std::vector<WindowedItem> &items, uint32_t stride)
{
   const auto entered = std::chrono::steady_clock::now();
   const char *debug = std::getenv("NFCGPU_WINDOW_DEBUG");
   WindowedSubmission W {config, stride, items, ctx->configs[config], (uint32_t)items.size(), debug != nullptr, debug ? std::atoi(debug) : 0, entered};
   int rc;

   if (ctx->tail)
   {
      W.under = !W.debugStages && may_overlap(ctx, config, items);

      if (!W.under && (rc = settle_tail(ctx)))
         return rc;
   }

   if (W.debugStages && ctx->pipeline && !ctx->inBlocks)
      std::fprintf(stderr, "[nfcgpu] the stage log is of unpipelined submissions: with NFCGPU_WINDOW_DEBUG set every submission is complete when its call returns\n");

   plan_scan_params(ctx, W);
   plan_tables(ctx, W);

   if (W.under && (rc = take_second_set(ctx, W)))
      return rc;

   if (!W.under && (rc = grow_front(ctx, W, false)))
      return without_the_memory(ctx, W, rc);

   fill_scan_args(ctx, W);

   if (W.under)
   {
      if ((rc = front(ctx, W, FrontPass {ctx->front, true, false})) || W.routed || (rc = join_front(ctx, W)) || W.routed)
         return rc;
   }
   else if ((rc = front(ctx, W, FrontPass {ctx->stream, false, false})) || W.routed)
      return rc;

   if ((rc = back_lane_buffers(ctx, W)) || W.routed || (rc = back_sink_and_save(ctx, W)) || W.routed || (rc = back_shadow_states(ctx, W)) ||
       (rc = back_place_windows(ctx, W)) || W.routed)
      return rc;

   return back_lanes_and_tail(ctx, W);
}


/* the next staging slot, idle and at least `bytes` large */
int stage_acquire(nfcgpu_ctx *ctx, size_t bytes, nfcgpu_ctx::StageSlot **out)
{
   nfcgpu_ctx::StageSlot &slot = ctx->stage[ctx->stageNext];
   ctx->stageNext ^= 1u;

   /* (the slot of the pending tail's submission - its turn comes round when a submission in between failed: the tail's kernels
    * still read the rows) */
   if (ctx->tail && ctx->tail->slot == &slot)
   {
      const int settled = settle_tail(ctx);
      if (settled)
         return settled;
   }

   if (slot.busy)
   {
      /* the launches of the submission before the last one: long done in a steady stream of submissions */
      HIP_TRY(ctx, hipEventSynchronize(slot.done));
      slot.busy = false;
   }

   if (!slot.done)
      HIP_TRY(ctx, hipEventCreateWithFlags(&slot.done, hipEventDisableTiming));

   if (bytes > slot.bytes)
   {
      if (slot.d)
         (void)hipFree(slot.d);
      if (slot.h)
         (void)hipHostFree(slot.h);

      slot.d = nullptr;
      slot.h = nullptr;
      slot.bytes = 0;

      const size_t want = bytes + bytes / 2;
      if (hipMalloc((void **)&slot.d, want) != hipSuccess)
         return fail(ctx, NFCGPU_ENOMEM, "staging buffer allocation failed");
      if (hipHostMalloc((void **)&slot.h, want, hipHostMallocDefault) != hipSuccess)
      {
         (void)hipFree(slot.d);
         slot.d = nullptr;
         return fail(ctx, NFCGPU_ENOMEM, "pinned staging buffer allocation failed");
      }

      slot.bytes = want;
   }

   *out = &slot;
   return NFCGPU_OK;
}

/* everything that reads the slot has been enqueued */
void stage_release(nfcgpu_ctx *ctx, nfcgpu_ctx::StageSlot *slot)
{
   if (slot && hipEventRecord(slot->done, ctx->stream) == hipSuccess)
      slot->busy = true;
   else if (slot)
      (void)hipStreamSynchronize(ctx->stream);
}

void drain_sink(nfcgpu_ctx *ctx, uint64_t cursor)
{
   const uint64_t valid = cursor < ctx->sinkWords ? cursor : ctx->sinkWords;
   uint64_t pos = 0;

   while (pos < valid && pos + NFC_FRAME_MAX_WORDS <= ctx->sinkWords)
   {
      const uint32_t *w = ctx->hSink.data() + pos;
      const uint32_t len = w[8] > NFC_STREAM_BYTES ? NFC_STREAM_BYTES : w[8];
      const uint32_t id = w[0];

      if (id < ctx->streams.size())
      {
         StreamInfo &si = ctx->streams[id];

         nfcgpu_frame f;
         std::memset(&f, 0, sizeof(f));
         f.stream_id = id;
         f.tech_type = w[1];
         f.frame_type = w[2];
         f.frame_flags = w[3];
         f.frame_phase = w[4];
         f.frame_rate = w[5];
         f.sample_start = w[6];
         f.sample_end = w[7];
         f.sample_rate = si.params.sample_rate;
         f.length = len;
         std::memcpy(f.data, w + NFC_FRAME_HEADER_WORDS, len);

         if (si.open)
            si.queue.push_back(f);

         ctx->stats.frames++;
      }

      pos += NFC_FRAME_HEADER_WORDS + ((len + 3) >> 2);
   }
}

}


/* ------------------------------------------------------------------------------------------ */
/* RCCL, looked up at run time (a host with a single GPU does not need it)                       */
/* ------------------------------------------------------------------------------------------ */
/* ncclUniqueId is passed by value: 128 bytes */
struct IdByValue
{
   char internal[NFCGPU_UNIQUE_ID_BYTES];
};

#ifdef NFCGPU_EMULATED_TEST_BUILD
struct FakeNcclId
{
   char internal[NFCGPU_UNIQUE_ID_BYTES];
};
extern "C" {
int fake_ncclGetUniqueId(void *id);
int fake_ncclCommInitRank(void **comm, int nRanks, FakeNcclId id, int rank);
int fake_ncclCommDestroy(void *comm);
int fake_ncclAllGather(const void *send, void *recv, size_t count, int type, void *comm, void *stream);
int fake_ncclBroadcast(const void *send, void *recv, size_t count, int type, int root, void *comm, void *stream);
int fake_ncclGroupStart();
int fake_ncclGroupEnd();
}
#endif

namespace {

struct Rccl
{
   void *handle = nullptr;
   int (*getUniqueId)(void *) = nullptr;
   int (*commInitRank)(void **, int, IdByValue, int) = nullptr;
   int (*commDestroy)(void *) = nullptr;
   int (*allGather)(const void *, void *, size_t, int, void *, hipStream_t) = nullptr;
   int (*broadcast)(const void *, void *, size_t, int, int, void *, hipStream_t) = nullptr;
   int (*groupStart)() = nullptr;
   int (*groupEnd)() = nullptr;
   const char *(*getErrorString)(int) = nullptr;
};

Rccl *rccl()
{
   static Rccl r;
   static bool tried = false;

   if (!tried)
   {
      tried = true;
#ifdef NFCGPU_EMULATED_TEST_BUILD
      /* the emulated test build has no RCCL; with NFCGPU_FAKE_RCCL=1 it takes an in-process stand-in (tests/hostsim/
       * fake_rccl.cpp: ranks are threads of one process) so that the rank logic of the gather runs without GPUs */
      if (std::getenv("NFCGPU_FAKE_RCCL"))
      {
         r.handle = (void *)&r;
         r.getUniqueId = fake_ncclGetUniqueId;
         r.commInitRank = (int (*)(void **, int, IdByValue, int))fake_ncclCommInitRank;
         r.commDestroy = fake_ncclCommDestroy;
         r.allGather = (int (*)(const void *, void *, size_t, int, void *, hipStream_t))fake_ncclAllGather;
         r.broadcast = (int (*)(const void *, void *, size_t, int, int, void *, hipStream_t))fake_ncclBroadcast;
         r.groupStart = fake_ncclGroupStart;
         r.groupEnd = fake_ncclGroupEnd;
         r.getErrorString = nullptr;
      }
#else
      for (const char *name: {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"})
      {
         r.handle = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
         if (r.handle)
            break;
      }

      if (r.handle)
      {
         r.getUniqueId = (int (*)(void *))dlsym(r.handle, "ncclGetUniqueId");
         r.commInitRank = (int (*)(void **, int, IdByValue, int))dlsym(r.handle, "ncclCommInitRank");
         r.commDestroy = (int (*)(void *))dlsym(r.handle, "ncclCommDestroy");
         r.allGather = (int (*)(const void *, void *, size_t, int, void *, hipStream_t))dlsym(r.handle, "ncclAllGather");
         r.broadcast = (int (*)(const void *, void *, size_t, int, int, void *, hipStream_t))dlsym(r.handle, "ncclBroadcast");
         r.groupStart = (int (*)())dlsym(r.handle, "ncclGroupStart");
         r.groupEnd = (int (*)())dlsym(r.handle, "ncclGroupEnd");
         r.getErrorString = (const char *(*)(int))dlsym(r.handle, "ncclGetErrorString");
      }
#endif
   }

   return (r.handle && r.getUniqueId && r.commInitRank && r.commDestroy && r.allGather && r.broadcast && r.groupStart && r.groupEnd) ? &r : nullptr;
}

}

namespace {

/* what a context owns besides the slots: streams, events, the work buffers of the time-parallel path */
void release_workspace(nfcgpu_ctx *ctx)
{
   if (ctx->stream)
      (void)hipStreamSynchronize(ctx->stream);
   if (ctx->side)
      (void)hipStreamSynchronize(ctx->side);
   if (ctx->low)
      (void)hipStreamSynchronize(ctx->low);
   if (ctx->front)
      (void)hipStreamSynchronize(ctx->front);

   for (auto *list: {&ctx->timed, &ctx->timedScan, &ctx->timedWindow, &ctx->timedWave, &ctx->timedPlanes})
   {
      for (auto &pl: *list)
      {
         (void)hipEventDestroy(pl.start);
         (void)hipEventDestroy(pl.stop);
      }
      list->clear();
   }
   for (auto e: ctx->eventPool)
      (void)hipEventDestroy(e);
   ctx->eventPool.clear();

   for (nfcgpu_ctx::DevBuf *b: {&ctx->wRepairs, &ctx->wRepairsEnv, &ctx->wJobs, &ctx->wChunks, &ctx->wPoints, &ctx->wSeams, &ctx->wChunkEdge, &ctx->wTiles, &ctx->wTileStats, &ctx->wWindows, &ctx->wRunList,
                                &ctx->wWorks, &ctx->wCounters, &ctx->vStates, &ctx->vCold, &ctx->vRings, &ctx->vBytes, &ctx->vSink, &ctx->vSinkCtl, &ctx->vSaveRings, &ctx->vSaveBytes,
                                &ctx->wPlanes, &ctx->wPlaneChunks, &ctx->wPlanesStale, &ctx->wShadow, &ctx->wShadowCtl})
   {
      if (b->ptr)
         (void)hipFree(b->ptr);
      b->ptr = nullptr;
      b->bytes = 0;
   }

   /* (the second set of pipelined submissions) */
   for (nfcgpu_ctx::DevBuf &b: ctx->otherSet)
   {
      if (b.ptr)
         (void)hipFree(b.ptr);
      b.ptr = nullptr;
      b.bytes = 0;
   }

   if (ctx->tailHost)
      (void)hipHostFree(ctx->tailHost);
   if (ctx->tailJobs)
      (void)hipHostFree(ctx->tailJobs);
   ctx->tailHost = ctx->frontHost = nullptr;
   ctx->tailJobs = nullptr;
   ctx->tailJobsBytes = 0;

   for (hipEvent_t *e: {&ctx->frontEvent, &ctx->planesFork, &ctx->planesJoin})
   {
      if (*e)
         (void)hipEventDestroy(*e);
      *e = nullptr;
   }
   if (ctx->front)
      (void)hipStreamDestroy(ctx->front);
   ctx->front = nullptr;

   if (ctx->epoch)
      (void)hipEventDestroy(ctx->epoch);
   ctx->epoch = nullptr;
   if (ctx->forkEvent)
      (void)hipEventDestroy(ctx->forkEvent);
   if (ctx->joinEvent)
      (void)hipEventDestroy(ctx->joinEvent);
   if (ctx->side)
      (void)hipStreamDestroy(ctx->side);
   if (ctx->low)
      (void)hipStreamDestroy(ctx->low);
   ctx->low = nullptr;
   if (ctx->stream)
      (void)hipStreamDestroy(ctx->stream);
   ctx->forkEvent = ctx->joinEvent = nullptr;
   ctx->side = ctx->stream = nullptr;
}

/* A profiled service that never resets its statistics must not collect a span per launch for ever: once the list is long, the
 * spans that end before the most recent ones begin - their union can no longer change - are folded into a running total. */
void fold_wave_spans(nfcgpu_ctx *ctx)
{
   std::vector<std::pair<float, float>> &v = ctx->waveSpans;

   if (v.size() < 4096)
      return;

   std::sort(v.begin(), v.end());

   /* the list becomes the union of its spans; an interval of that union that ends before the most recent 64 spans begin can
    * no longer grow (launches of one submission overlap, those of different submissions do not) and goes into the total */
   const float horizon = v[v.size() - 64].first;
   std::vector<std::pair<float, float>> open;
   double busy = 0.0;
   float lo = v[0].first, hi = v[0].second;

   for (size_t i = 1; i < v.size(); i++)
   {
      if (v[i].first > hi)
      {
         if (hi < horizon)
            busy += hi - lo;
         else
            open.push_back(std::make_pair(lo, hi));
         lo = v[i].first;
         hi = v[i].second;
      }
      else if (v[i].second > hi)
         hi = v[i].second;
   }

   open.push_back(std::make_pair(lo, hi));

   ctx->waveBusyMs += busy;
   v.swap(open);
}

/* HIP-event spans recorded since the last call -> milliseconds in the context's statistics; the events go back to the pool.
 * The streams the events were recorded on must have been waited for. */
void collect_timings(nfcgpu_ctx *ctx)
{
   struct Into
   {
      std::vector<ProfiledLaunch> *list;
      double *ms;
      uint64_t *count;
   } all[] = {{&ctx->timed, &ctx->stats.kernel_ms, nullptr},
              {&ctx->timedScan, &ctx->stats.scan_ms, nullptr},
              {&ctx->timedWindow, &ctx->stats.window_ms, nullptr},
              {&ctx->timedWave, &ctx->stats.wave_ms, &ctx->stats.wave_launches},
              {&ctx->timedPlanes, &ctx->stats.planes_ms, nullptr}};

   for (Into &into: all)
   {
      for (auto &pl: *into.list)
      {
         float ms = 0;
         if (hipEventElapsedTime(&ms, pl.start, pl.stop) == hipSuccess)
         {
            *into.ms += ms;
            if (into.count)
               ++*into.count;

            /* the wave decoder's launches run on two streams side by side: where they lie in time, for the time the kernel
             * was running at all (nfcgpu_stats::wave_busy_ms) */
            float at = 0;
            if (into.list == &ctx->timedWave && ctx->epoch && hipEventElapsedTime(&at, ctx->epoch, pl.start) == hipSuccess)
               ctx->waveSpans.push_back(std::make_pair(at, at + ms));
         }
         ctx->eventPool.push_back(pl.start);
         ctx->eventPool.push_back(pl.stop);
      }
      into.list->clear();
   }

   fold_wave_spans(ctx);
}

int run_rows(nfcgpu_ctx *ctx, uint32_t first, uint32_t count, const uint8_t *devBase, uint64_t devPitch, uint32_t n, uint32_t stride);

}

extern "C" {

void nfcgpu_default_params(nfcgpu_params *p)
{
   if (!p)
      return;

   std::memset(p, 0, sizeof(*p));
   p->sample_rate = 0;
   p->tech_mask = NFCGPU_TECH_A | NFCGPU_TECH_B | NFCGPU_TECH_F | NFCGPU_TECH_V;
   p->power_level_threshold = 0.01f;

   const float corr[4] = {0.75f, 0.50f, 0.50f, 0.50f};
   const float lo[4] = {0.90f, 0.10f, 0.10f, 0.90f};
   const float hi[4] = {1.00f, 0.90f, 0.90f, 1.00f};

   for (int t = 0; t < 4; t++)
   {
      p->corr_threshold[t] = corr[t];
      p->min_modulation_depth[t] = lo[t];
      p->max_modulation_depth[t] = hi[t];
   }
}

int nfcgpu_init(int device, const nfcgpu_options *options, nfcgpu_ctx **out)
{
   if (!out)
      return NFCGPU_EINVAL;

   *out = nullptr;

   int count = 0;
   if (hipGetDeviceCount(&count) != hipSuccess || count <= 0 || device < 0 || device >= count)
      return NFCGPU_ENODEV;

   if (hipSetDevice(device) != hipSuccess)
      return NFCGPU_ENODEV;

   nfcgpu_ctx *ctx = new (std::nothrow) nfcgpu_ctx();
   if (!ctx)
      return NFCGPU_ENOMEM;

   ctx->device = device;

   const char *generic = std::getenv("NFCGPU_GENERIC_KERNELS");
   ctx->genericOnly = generic && generic[0] == '1';

   /* Tuning switches of the time-parallel path. They are experiment switches, not configuration (round 6: the product library
    * used to read all nineteen from the environment): libnfcgpu.so runs on the defaults of nfcgpu_ctx and does not look at them.
    * A build of this file with -DNFCGPU_TUNING_KNOBS (`make tuning`: libnfcgpu_tuning.so, the same kernels; and the emulated test
    * build) takes them from the environment - what the tests use to force every path on small inputs and what the sweeps under
    * profiles/ were made with. What the product reads: NFCGPU_WINDOW_DEBUG (stage log on stderr), NFCGPU_GENERIC_KERNELS (the
    * any-rate kernels at the compiled-in rate too) and, in the shim, NFCGPU_DEVICE / NFCGPU_MAX_STREAMS / NFCGPU_SHIM_BLOCK(_MS). */
#if defined(NFCGPU_TUNING_KNOBS) || defined(NFCGPU_EMULATED_TEST_BUILD)
   auto tuning = [](const char *name) -> const char * { return std::getenv(name); };
#else
   auto tuning = [](const char *) -> const char * { return nullptr; };
#endif
   auto knob = [&](const char *name, uint32_t fallback) -> uint32_t {
      const char *v = tuning(name);
      return v && v[0] ? (uint32_t)std::strtoul(v, nullptr, 10) : fallback;
   };

   ctx->windowed = knob("NFCGPU_WINDOWED", 1) != 0;
   ctx->windowedMinSamples = knob("NFCGPU_WINDOWED_MIN", ctx->windowedMinSamples);
   ctx->scanChunkFixed = tuning("NFCGPU_SCAN_CHUNK") != nullptr && tuning("NFCGPU_SCAN_CHUNK")[0] != 0;
   ctx->scanChunk = knob("NFCGPU_SCAN_CHUNK", ctx->scanChunk) / NFC_SCAN_POINT * NFC_SCAN_POINT;
   ctx->scanLanes = knob("NFCGPU_SCAN_LANES", ctx->scanLanes);
   if (ctx->scanLanes == 0u)
      ctx->scanLanes = 1u;
   ctx->scanWarm = knob("NFCGPU_SCAN_WARM", ctx->scanWarm) / NFC_SCAN_POINT * NFC_SCAN_POINT;
   ctx->maxPasses = knob("NFCGPU_WINDOW_PASSES", ctx->maxPasses);
   ctx->maxPassesFew = knob("NFCGPU_WINDOW_PASSES_FEW", knob("NFCGPU_WINDOW_PASSES", ctx->maxPassesFew));
   ctx->soloSamples = knob("NFCGPU_SOLO_SAMPLES", ctx->soloSamples);
   ctx->stagingWords = knob("NFCGPU_STAGING_WORDS", ctx->stagingWords);
   ctx->lanesWanted = knob("NFCGPU_LANES_WANTED", ctx->lanesWanted);
   ctx->longFirst = knob("NFCGPU_LONG_FIRST", ctx->longFirst);
   ctx->envelopeMax = knob("NFCGPU_ENVELOPE_KERNEL", ctx->envelopeMax);
   ctx->envelopeFollowMax = knob("NFCGPU_ENVELOPE_FOLLOW", ctx->envelopeFollowMax);
   ctx->planesPiece = knob("NFCGPU_PLANES_PIECE", ctx->planesPiece);
   ctx->planesBeside = knob("NFCGPU_PLANES_BESIDE", ctx->planesBeside);
   ctx->planesBesidePiece = knob("NFCGPU_PLANES_BESIDE_PIECE", ctx->planesBesidePiece);
   ctx->cutMax = knob("NFCGPU_CUT_MAX", ctx->cutMax);
   if (ctx->cutMax < NFC_WINDOW_CUT)
      ctx->cutMax = NFC_WINDOW_CUT;
   ctx->sideMode = knob("NFCGPU_SIDE_STREAM", ctx->sideMode);
   ctx->pipeline = knob("NFCGPU_PIPELINE", 1) != 0;
   ctx->spoilShadow = knob("NFCGPU_TEST_SPOIL_SHADOW", 0);
   ctx->dumpWindows = tuning("NFCGPU_DUMP_WINDOWS") != nullptr;
   ctx->pipelineReport = tuning("NFCGPU_PIPELINE_REPORT") != nullptr;
   ctx->blockSamples = knob("NFCGPU_BLOCK_SAMPLES", ctx->blockSamples) / NFC_SCAN_POINT * NFC_SCAN_POINT;
   if (ctx->blockSamples < 65536u)
      ctx->blockSamples = 65536u;

   if (ctx->scanWarm < NFC_SCAN_POINT)
      ctx->scanWarm = NFC_SCAN_POINT;
   if (ctx->scanChunk < ctx->scanWarm + NFC_SCAN_POINT)
      ctx->scanChunk = ctx->scanWarm + NFC_SCAN_POINT;

   uint32_t maxStreams = options && options->max_streams ? options->max_streams : 1024;
   uint64_t sinkBytes = options && options->frame_sink_bytes ? options->frame_sink_bytes : (64ull << 20);

   maxStreams = (maxStreams + NFC_LANES - 1) / NFC_LANES * NFC_LANES;

   if (sinkBytes < 4ull * 4 * NFC_FRAME_MAX_WORDS)
      sinkBytes = 4ull * 4 * NFC_FRAME_MAX_WORDS;
   if (sinkBytes > (0xFFFFFFF0ull * 4ull))
      sinkBytes = 0xFFFFFFF0ull * 4ull;

   ctx->maxStreams = maxStreams;
   ctx->blocks = maxStreams / NFC_LANES;
   ctx->sinkWords = sinkBytes / 4;

   bool ok = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) == hipSuccess;
   ok = ok && hipStreamCreateWithFlags(&ctx->side, hipStreamNonBlocking) == hipSuccess;
   {
      /* (the stream of the walk that writes the planes beside the rounds of second walks: whatever those rounds launch goes first) */
      int least = 0, greatest = 0;
      if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess)
         least = 0;
      ok = ok && hipStreamCreateWithPriority(&ctx->low, hipStreamNonBlocking, least) == hipSuccess;
   }
   ok = ok && hipEventCreateWithFlags(&ctx->forkEvent, hipEventDisableTiming) == hipSuccess;
   ok = ok && hipEventCreateWithFlags(&ctx->joinEvent, hipEventDisableTiming) == hipSuccess;
   /* pipelined submissions: the stream of a front that runs under the tail of the submission before, its events, the pinned words
    * of the read-backs */
   ok = ok && hipStreamCreateWithFlags(&ctx->front, hipStreamNonBlocking) == hipSuccess;
   ok = ok && hipEventCreateWithFlags(&ctx->frontEvent, hipEventDisableTiming) == hipSuccess;
   ok = ok && hipEventCreateWithFlags(&ctx->planesFork, hipEventDisableTiming) == hipSuccess;
   ok = ok && hipEventCreateWithFlags(&ctx->planesJoin, hipEventDisableTiming) == hipSuccess;
   ok = ok && hipHostMalloc((void **)&ctx->tailHost, 64 * sizeof(uint32_t), hipHostMallocDefault) == hipSuccess;
   if (ok)
   {
      std::memset(ctx->tailHost, 0, 64 * sizeof(uint32_t));
      ctx->frontHost = ctx->tailHost + 32;
   }

   ok = ok && hipMalloc((void **)&ctx->dStates, sizeof(NfcStreamState) * (size_t)maxStreams) == hipSuccess;
   ok = ok && hipMalloc((void **)&ctx->dCold, sizeof(NfcStreamCold) * (size_t)maxStreams) == hipSuccess;
   ok = ok && hipMalloc((void **)&ctx->dRings, sizeof(float) * (size_t)kRingBlockFloats * ctx->blocks) == hipSuccess;
   ok = ok && hipMalloc((void **)&ctx->dBytes, (size_t)NFC_STREAM_BYTES * maxStreams) == hipSuccess;
   ok = ok && hipMalloc((void **)&ctx->dSink, ctx->sinkWords * 4) == hipSuccess;
   ok = ok && hipMalloc((void **)&ctx->dSinkCtl, 16) == hipSuccess;
   ok = ok && hipMalloc((void **)&ctx->dWorks, sizeof(NfcWork) * (size_t)maxStreams) == hipSuccess;
   ok = ok && hipMalloc((void **)&ctx->dConfigs, sizeof(NfcConfig) * kMaxConfigs) == hipSuccess;

   if (ok)
   {
      ok = ok && hipMemsetAsync(ctx->dStates, 0, sizeof(NfcStreamState) * (size_t)maxStreams, ctx->stream) == hipSuccess;
      ok = ok && hipMemsetAsync(ctx->dCold, 0, sizeof(NfcStreamCold) * (size_t)maxStreams, ctx->stream) == hipSuccess;
      ok = ok && hipMemsetAsync(ctx->dRings, 0, sizeof(float) * (size_t)kRingBlockFloats * ctx->blocks, ctx->stream) == hipSuccess;
      ok = ok && hipMemsetAsync(ctx->dBytes, 0, (size_t)NFC_STREAM_BYTES * maxStreams, ctx->stream) == hipSuccess;
      ok = ok && hipMemsetAsync(ctx->dSinkCtl, 0, 16, ctx->stream) == hipSuccess;
      ok = ok && hipStreamSynchronize(ctx->stream) == hipSuccess;
   }

   if (!ok)
   {
      nfcgpu_shutdown(ctx);
      return NFCGPU_ENOMEM;
   }

   ctx->ownSink = ctx->dSink;
   ctx->ownSinkCtl = ctx->dSinkCtl;
   ctx->ownSinkWords = ctx->sinkWords;

   ctx->streams.resize(maxStreams);
   ctx->hWorks.resize(maxStreams);
   for (auto &w: ctx->hWorks)
   {
      w.data = nullptr;
      w.count = 0;
      w.stride = 1;
   }

   *out = ctx;
   return NFCGPU_OK;
}

int nfcgpu_shutdown(nfcgpu_ctx *ctx)
{
   if (!ctx)
      return NFCGPU_EINVAL;

   (void)hipSetDevice(ctx->device);

   (void)settle_tail(ctx);

   if (ctx->stream)
      (void)hipStreamSynchronize(ctx->stream);
   if (ctx->side)
      (void)hipStreamSynchronize(ctx->side); /* (nothing of its work may outlive the buffers freed below) */

   (void)hipFree(ctx->dStates);
   (void)hipFree(ctx->dCold);
   (void)hipFree(ctx->dRings);
   (void)hipFree(ctx->dBytes);
   (void)hipFree(ctx->ownSink ? ctx->ownSink : ctx->dSink);
   (void)hipFree(ctx->ownSinkCtl ? ctx->ownSinkCtl : ctx->dSinkCtl);
   (void)hipFree(ctx->dWorks);
   (void)hipFree(ctx->dConfigs);
   for (nfcgpu_ctx::SpectrumTables &t: ctx->spectrumTables)
      (void)hipFree(t.d);
   if (ctx->recordPartials)
      (void)hipFree(ctx->recordPartials);
   if (ctx->tapScratch)
      (void)hipFree(ctx->tapScratch);
   if (ctx->tapCount)
      (void)hipHostFree(ctx->tapCount);
   if (ctx->tapReduceScratch)
      (void)hipFree(ctx->tapReduceScratch);
   if (ctx->apcmScratch)
      (void)hipFree(ctx->apcmScratch);
   for (nfcgpu_ctx::StageSlot &slot: ctx->stage)
   {
      if (slot.d)
         (void)hipFree(slot.d);
      if (slot.h)
         (void)hipHostFree(slot.h);
      if (slot.done)
         (void)hipEventDestroy(slot.done);
   }

   nfcgpu_comm_destroy(ctx);

   release_workspace(ctx);

   delete ctx;
   return NFCGPU_OK;
}

int nfcgpu_stream_open_many(nfcgpu_ctx *ctx, const nfcgpu_params *params, uint32_t count, uint32_t *first)
{
   SETTLE_FIRST(ctx);

   if (!ctx || !first || count == 0)
      return NFCGPU_EINVAL;


   /* first fit of `count` contiguous free slots */
   uint32_t run = 0, start = 0;
   bool found = false;

   for (uint32_t i = 0; i < ctx->maxStreams; i++)
   {
      if (ctx->streams[i].open)
      {
         run = 0;
         continue;
      }
      if (run == 0)
         start = i;
      if (++run == count)
      {
         found = true;
         break;
      }
   }

   if (!found)
      return fail(ctx, NFCGPU_EFULL, "no free stream slots (raise nfcgpu_options.max_streams)");

   nfcgpu_params p;
   if (params)
      p = *params;
   else
      nfcgpu_default_params(&p);

   for (uint32_t i = start; i < start + count; i++)
   {
      StreamInfo &si = ctx->streams[i];
      si = StreamInfo();
      si.open = true;
      si.params = p;
      si.powerAtInit = p.power_level_threshold;
   }

   *first = start;
   return NFCGPU_OK;
}

int nfcgpu_stream_open(nfcgpu_ctx *ctx, const nfcgpu_params *params, uint32_t *id)
{
   return nfcgpu_stream_open_many(ctx, params, 1, id);
}

int nfcgpu_stream_configure(nfcgpu_ctx *ctx, uint32_t id, const nfcgpu_params *params)
{
   SETTLE_FIRST(ctx);

   if (!ctx || !params)
      return NFCGPU_EINVAL;

   if (id >= ctx->maxStreams || !ctx->streams[id].open)
      return fail(ctx, NFCGPU_ESTREAM, "unknown stream");

   StreamInfo &si = ctx->streams[id];
   const uint32_t oldRate = si.params.sample_rate;

   if (params->sample_rate != 0 && params->sample_rate != oldRate && oldRate != 0 && ctx->dirty && !ctx->hold)
   {
      /* frames already produced keep the rate stored when they were produced */
      int rc = nfcgpu_sync(ctx);
      if (rc != NFCGPU_OK && rc != NFCGPU_EOVERFLOW)
         return rc;
   }

   si.params = *params;

   /* setSampleRate() only stores the value (0 = leave it alone); nothing is re-derived from it until the decoder
    * (re)initialises, see adopt_sample_rate */
   if (params->sample_rate == 0)
      si.params.sample_rate = oldRate;

   if (si.initialized && !si.needInit)
      return resolve_config(ctx, si); /* thresholds and the enable mask take effect immediately */

   return NFCGPU_OK;
}

int nfcgpu_stream_reset(nfcgpu_ctx *ctx, uint32_t id)
{
   SETTLE_FIRST(ctx);

   if (!ctx)
      return NFCGPU_EINVAL;

   if (id >= ctx->maxStreams || !ctx->streams[id].open)
      return fail(ctx, NFCGPU_ESTREAM, "unknown stream");

   /* initialize(): everything is derived again from what is stored now (applied when the next buffer arrives) */
   StreamInfo &si = ctx->streams[id];
   si.needInit = true;
   si.explicitInit = true;
   si.derivedRate = si.params.sample_rate;
   si.powerAtInit = si.params.power_level_threshold;
   return NFCGPU_OK;
}

int nfcgpu_stream_close(nfcgpu_ctx *ctx, uint32_t id)
{
   SETTLE_FIRST(ctx);

   if (!ctx)
      return NFCGPU_EINVAL;

   if (id >= ctx->maxStreams || !ctx->streams[id].open)
      return fail(ctx, NFCGPU_ESTREAM, "unknown stream");

   int rc = nfcgpu_sync(ctx);

   ctx->streams[id] = StreamInfo();
   return rc;
}

#ifdef NFCGPU_EMULATED_TEST_BUILD
namespace {

/* TEST SCAFFOLDING, emulated build only. The CPU twins of the kernels (tests/hostsim) read floats and nothing else, so here the
 * _fmt entry points widen an int16 buffer on the host - nfc_i16_to_float, the conversion the device loaders apply - and go on as
 * NFCGPU_FMT_F32. What the emulated build therefore exercises of int16 input is the argument checks, the rate adoption and the
 * equality of the conversion; what it does not: the device loaders (nfc_sample_at, the int16 row fetches of nfc_stage_tile,
 * nfc_scan_body and nfc_planes_body), the slice offsets in bytes per sample and the staging sizes. Those run on the GPU only
 * (tests/test_int16_input.py there). The floats live until the next nfcgpu_sync, as device-resident input has to. */
const float *widen_i16(nfcgpu_ctx *ctx, const void *data, size_t values)
{
   ctx->widened.emplace_back(values ? values : 1);
   std::vector<float> &to = ctx->widened.back();
   for (size_t i = 0; i < values; i++)
      to[i] = nfc_i16_to_float(((const int16_t *)data)[i]);
   return to.data();
}

}
#endif

int nfcgpu_submit_batch_fmt(nfcgpu_ctx *ctx, const nfcgpu_batch *b, uint32_t format)
{
   SETTLE_FIRST(ctx);

   if (!ctx || !b || !b->stream_ids || !b->data || !b->n_samples || (b->stride != 1 && b->stride != 2) ||
       (b->location != NFCGPU_LOC_HOST && b->location != NFCGPU_LOC_DEVICE) || (format != NFCGPU_FMT_F32 && format != NFCGPU_FMT_I16))
      return NFCGPU_EINVAL;

   /* the sample layout of the batch (nfc_sample.hpp): b->stride itself for floats */
   const uint32_t layout = b->stride | (format == NFCGPU_FMT_I16 ? NFC_SAMPLE_I16 : 0u);

   if (format == NFCGPU_FMT_I16)
   {
      /* rows are read as int16 or as pairs of them: every pointer has to be aligned to a sample */
      for (uint32_t i = 0; i < b->n_streams; i++)
      {
         if (((uintptr_t)b->data[i] % nfc_sample_bytes(layout)) != 0)
            return fail(ctx, NFCGPU_EINVAL, "int16 data pointers must be multiples of the sample size (2 bytes magnitude, 4 bytes IQ)");
      }

#ifdef NFCGPU_EMULATED_TEST_BUILD
      /* (test scaffolding: see widen_i16) */
      std::vector<const void *> rows(b->n_streams);
      for (uint32_t i = 0; i < b->n_streams; i++)
         rows[i] = b->data[i] ? widen_i16(ctx, b->data[i], (size_t)b->n_samples[i] * b->stride) : nullptr;

      nfcgpu_batch wide = *b;
      wide.data = rows.data();
      return nfcgpu_submit_batch_fmt(ctx, &wide, NFCGPU_FMT_F32);
#endif
   }

   if (b->n_streams == 0)
      return NFCGPU_OK;

   HIP_TRY(ctx, hipSetDevice(ctx->device));

   /* the per-slot work table and the batch marks are idle between calls: every exit path restores that */
   auto clearWorks = [&]() {
      for (uint32_t i = 0; i < b->n_streams; i++)
      {
         const uint32_t id = b->stream_ids[i];
         if (id >= ctx->maxStreams)
            continue;
         NfcWork &w = ctx->hWorks[id];
         w.data = nullptr;
         w.count = 0;
         w.stride = 1;
         ctx->streams[id].listed = false;
      }
   };

   /* validate + adopt rate */
   size_t hostBytes = 0;
   uint32_t lo = 0xFFFFFFFFu, hi = 0;
   int rc = NFCGPU_OK;

   for (uint32_t i = 0; i < b->n_streams && rc == NFCGPU_OK; i++)
   {
      const uint32_t id = b->stream_ids[i];

      if (id >= ctx->maxStreams || !ctx->streams[id].open)
         rc = fail(ctx, NFCGPU_ESTREAM, "unknown stream in batch");
      else if (ctx->streams[id].listed)
         rc = fail(ctx, NFCGPU_EINVAL, "stream listed twice in one batch");
      else if (b->n_samples[i] && !b->data[i])
         rc = fail(ctx, NFCGPU_EINVAL, "null data pointer in batch");
      else
         rc = adopt_sample_rate(ctx, ctx->streams[id], b->sample_rate);

      if (rc)
         break;

      ctx->streams[id].listed = true;
      ctx->hWorks[id].count = b->n_samples[i];
      hostBytes += (size_t)b->n_samples[i] * nfc_sample_bytes(layout);
      lo = id < lo ? id : lo;
      hi = id > hi ? id : hi;
   }

   if (rc)
   {
      clearWorks();
      return rc;
   }

   /* one launch per decoder configuration present in the batch */
   std::vector<uint32_t> cfgs;
   for (uint32_t i = 0; i < b->n_streams; i++)
   {
      uint32_t c = ctx->streams[b->stream_ids[i]].config;
      bool seen = false;
      for (uint32_t k: cfgs)
         seen = seen || k == c;
      if (!seen)
         cfgs.push_back(c);
   }

   /* staging slot: the samples (host batches) and one work table per configuration group, all sent from pinned memory
    * so that nothing the copies read belongs to this call's stack or to the caller once it returns */
   const size_t tableBytes = (sizeof(NfcWork) * (size_t)(hi - lo + 1) + 255) & ~(size_t)255;
   nfcgpu_ctx::StageSlot *slot = nullptr;

   rc = stage_acquire(ctx, (b->location == NFCGPU_LOC_HOST ? hostBytes + 256 * (size_t)b->n_streams : 0) + tableBytes * (cfgs.size() + 1) + 256, &slot);
   if (rc)
   {
      clearWorks();
      return rc;
   }

   ctx->inflight = true;

   /* from here on every exit records the slot's event behind whatever has been enqueued */
   struct Release
   {
      nfcgpu_ctx *ctx;
      nfcgpu_ctx::StageSlot *slot;
      ~Release() { stage_release(ctx, slot); }
   } release {ctx, slot};

   rc = initialize_pending(ctx, lo, hi - lo + 1, true);
   if (rc)
   {
      clearWorks();
      return rc;
   }

   size_t stageAt = 0;

   for (uint32_t i = 0; i < b->n_streams; i++)
   {
      const uint32_t id = b->stream_ids[i];
      NfcWork &w = ctx->hWorks[id];
      const size_t bytes = (size_t)b->n_samples[i] * nfc_sample_bytes(layout);

      w.stride = layout;

      if (b->location == NFCGPU_LOC_HOST)
      {
         w.data = slot->d + stageAt;
         if (bytes)
            std::memcpy(slot->h + stageAt, b->data[i], bytes);
         stageAt += (bytes + 255) & ~(size_t)255;
      }
      else
      {
         w.data = (const uint8_t *)b->data[i];
      }
   }

   if (stageAt)
   {
      hipError_t err = hipMemcpyAsync(slot->d, slot->h, stageAt, hipMemcpyHostToDevice, ctx->stream);
      if (err != hipSuccess)
      {
         clearWorks();
         return fail(ctx, NFCGPU_EHIP, "hipMemcpyAsync(H2D samples)", err);
      }
   }

   size_t tableAt = (stageAt + 255) & ~(size_t)255; /* the groups' work tables follow the samples in the pinned mirror */

   for (uint32_t c: cfgs)
   {
      {
         std::vector<WindowedItem> items;
         for (uint32_t i = 0; i < b->n_streams; i++)
         {
            const uint32_t id = b->stream_ids[i];
            if (ctx->streams[id].config == c)
               items.push_back(WindowedItem {id, ctx->hWorks[id].data, b->n_samples[i]});
         }

         if (windowed_eligible(ctx, c, items))
         {
            rc = run_windowed(ctx, c, items, layout);
            if (rc)
            {
               clearWorks();
               return rc;
            }
            continue;
         }
      }

      uint32_t first = 0xFFFFFFFFu, last = 0;
      uint64_t groupSamples = 0;
      bool exactPossible = false, exactOnly = true;

      for (uint32_t i = 0; i < b->n_streams; i++)
      {
         const uint32_t id = b->stream_ids[i];
         if (ctx->streams[id].config != c)
            continue;
         first = id < first ? id : first;
         last = id > last ? id : last;
         groupSamples += b->n_samples[i];
         const bool exact = exact_zone(ctx->streams[id].clock, b->n_samples[i]);
         exactPossible = exactPossible || exact;
         exactOnly = exactOnly && (exact || b->n_samples[i] == 0);
      }

      /* slots of other configurations inside [first,last] must stay idle in this launch */
      NfcWork *table = (NfcWork *)(slot->h + tableAt);
      const size_t entries = (size_t)last - first + 1;
      tableAt += tableBytes;

      for (uint32_t id = first; id <= last; id++)
      {
         table[id - first] = ctx->hWorks[id];

         if (!ctx->streams[id].open || ctx->streams[id].config != c)
         {
            table[id - first].data = nullptr;
            table[id - first].count = 0;
            table[id - first].stride = 1;
         }
      }

      /* (stream order: the copy lands after the launch of the group before has finished with the device table) */
      hipError_t err = hipMemcpyAsync(ctx->dWorks + first, table, sizeof(NfcWork) * entries, hipMemcpyHostToDevice, ctx->stream);
      if (err != hipSuccess)
      {
         clearWorks();
         return fail(ctx, NFCGPU_EHIP, "hipMemcpyAsync(work table)", err);
      }

      NfcLaunch L = base_launch(ctx);
      L.works = ctx->dWorks;
      L.uniformStride = layout; /* one sample format per batch */
      L.firstSlot = first;
      L.slotCount = last - first + 1;

      rc = launch_demod(ctx, c, L, groupSamples, exactPossible, exactOnly);
      if (rc)
      {
         clearWorks();
         return rc;
      }

      /* the clock mirrors follow once the launch is on its way */
      for (uint32_t i = 0; i < b->n_streams; i++)
      {
         const uint32_t id = b->stream_ids[i];
         if (ctx->streams[id].config == c)
            commit_clock(ctx->streams[id], b->n_samples[i]);
      }
   }

   /* no wait: the staging slot and its tables are protected by the slot's event (stage_release), the results are
    * collected by whoever asks for them (nfcgpu_sync / poll / flush) */
   clearWorks();
   return NFCGPU_OK;
}

int nfcgpu_submit_batch(nfcgpu_ctx *ctx, const nfcgpu_batch *b)
{
   return nfcgpu_submit_batch_fmt(ctx, b, NFCGPU_FMT_F32);
}

int nfcgpu_submit(nfcgpu_ctx *ctx, uint32_t id, const float *data, uint32_t n, uint32_t stride, uint32_t sampleRate)
{
   return nfcgpu_submit_fmt(ctx, id, data, n, stride, sampleRate, NFCGPU_FMT_F32);
}

int nfcgpu_submit_fmt(nfcgpu_ctx *ctx, uint32_t id, const void *data, uint32_t n, uint32_t stride, uint32_t sampleRate, uint32_t format)
{
   const void *ptr = data;
   nfcgpu_batch b;
   std::memset(&b, 0, sizeof(b));
   b.n_streams = 1;
   b.stride = stride;
   b.location = NFCGPU_LOC_HOST;
   b.sample_rate = sampleRate;
   b.stream_ids = &id;
   b.data = &ptr;
   b.n_samples = &n;
   return nfcgpu_submit_batch_fmt(ctx, &b, format);
}

int nfcgpu_magnitude(nfcgpu_ctx *ctx, const float *iq, uint64_t n, float *out, uint32_t location)
{
   return nfcgpu_magnitude_fmt(ctx, iq, n, out, location, NFCGPU_FMT_F32);
}

int nfcgpu_magnitude_fmt(nfcgpu_ctx *ctx, const void *iq, uint64_t n, float *out, uint32_t location, uint32_t format)
{
   SETTLE_FIRST(ctx);

   if (!ctx || !iq || !out || (location != NFCGPU_LOC_HOST && location != NFCGPU_LOC_DEVICE) || (format != NFCGPU_FMT_F32 && format != NFCGPU_FMT_I16))
      return NFCGPU_EINVAL;

   const bool i16 = format == NFCGPU_FMT_I16;

   if (i16 && ((uintptr_t)iq % 4u) != 0)
      return fail(ctx, NFCGPU_EINVAL, "int16 IQ must be 4-byte aligned");

   if (n == 0)
      return NFCGPU_OK;

#ifdef NFCGPU_EMULATED_TEST_BUILD
   /* (test scaffolding: see widen_i16; the call waits, so the floats go at once) */
   if (i16)
   {
      const float *wide = widen_i16(ctx, iq, (size_t)n * 2);
      const int rc = nfcgpu_magnitude_fmt(ctx, wide, n, out, location, NFCGPU_FMT_F32);
      ctx->widened.pop_back();
      return rc;
   }
#endif

   HIP_TRY(ctx, hipSetDevice(ctx->device));

   const void *src = iq;
   float *dst = out;
   nfcgpu_ctx::StageSlot *slot = nullptr;

   ctx->inflight = true;

   if (location == NFCGPU_LOC_HOST)
   {
      /* staging area: IQ first, magnitudes behind it */
      const size_t inBytes = (size_t)n * (i16 ? 4 : 8), outBytes = (size_t)n * 4;
      int rc = stage_acquire(ctx, inBytes + outBytes, &slot);
      if (rc)
         return rc;

      std::memcpy(slot->h, iq, inBytes);
      HIP_TRY(ctx, hipMemcpyAsync(slot->d, slot->h, inBytes, hipMemcpyHostToDevice, ctx->stream));
      src = slot->d;
      dst = (float *)(slot->d + inBytes);
   }

   const uint32_t threads = 256;
   const uint64_t wanted = (n + threads - 1) / threads;
   const uint32_t grid = (uint32_t)(wanted < 16384 ? wanted : 16384);

#ifndef NFCGPU_EMULATED_TEST_BUILD
   if (i16)
      hipLaunchKernelGGL(nfc_magnitude_kernel_i16, dim3(grid), dim3(threads), 0, ctx->stream, (const NfcIq16 *)src, dst, n);
   else
#endif
      hipLaunchKernelGGL(nfc_magnitude_kernel, dim3(grid), dim3(threads), 0, ctx->stream, (const float2 *)src, dst, n);
   HIP_TRY(ctx, hipGetLastError());

   /* (the magnitudes sit behind the IQ in both halves of the slot) */
   const size_t outAt = (size_t)n * (i16 ? 4 : 8);

   if (location == NFCGPU_LOC_HOST)
      HIP_TRY(ctx, hipMemcpyAsync(slot->h + outAt, dst, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));

   /* the result goes back to the caller: this entry point waits */
   HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));

   if (location == NFCGPU_LOC_HOST)
      std::memcpy(out, slot->h + outAt, (size_t)n * 4);

   return NFCGPU_OK;
}

int nfcgpu_resample_radio(nfcgpu_ctx *ctx, const float *in, uint64_t inPitch, uint32_t nBuffers, uint32_t n, float *out, uint64_t outPitch,
                          uint32_t capacityPairs, uint32_t *counts, uint32_t location)
{
   SETTLE_FIRST(ctx);

   if (!ctx || !in || !out || !counts || n < 25 || (inPitch & 3) || (outPitch & 7) || ((uintptr_t)out & 7) || inPitch < (uint64_t)n * 4 ||
       outPitch < (uint64_t)capacityPairs * 8 || (location != NFCGPU_LOC_HOST && location != NFCGPU_LOC_DEVICE))
      return NFCGPU_EINVAL;
   if (nBuffers == 0)
      return NFCGPU_OK;

   HIP_TRY(ctx, hipSetDevice(ctx->device));

   const float *dIn = in;
   float *dOut = out;
   uint32_t *dCounts = counts;
   uint8_t *scratch = nullptr;
   std::vector<uint32_t> hostCounts;

   const size_t inBytes = (size_t)inPitch * nBuffers, outBytes = (size_t)outPitch * nBuffers, cntBytes = (size_t)nBuffers * 4;

   if (location == NFCGPU_LOC_HOST)
   {
      /* one temporary device block: input, output, counts (this entry point is not on the streaming path) */
      if (hipMalloc((void **)&scratch, inBytes + outBytes + cntBytes) != hipSuccess)
         return fail(ctx, NFCGPU_ENOMEM, "resampler scratch allocation failed");

      hipError_t err = hipMemcpy(scratch, in, inBytes, hipMemcpyHostToDevice);
      if (err != hipSuccess)
      {
         (void)hipFree(scratch);
         return fail(ctx, NFCGPU_EHIP, "hipMemcpy(H2D resampler input)", err);
      }

      dIn = (const float *)scratch;
      dOut = (float *)(scratch + inBytes);
      dCounts = (uint32_t *)(scratch + inBytes + outBytes);
   }

   hipLaunchKernelGGL(nfc_resample_radio_kernel, dim3((nBuffers + NFC_LANES - 1) / NFC_LANES), dim3(NFC_LANES), 0, ctx->stream, dIn,
                      inPitch / 4, nBuffers, n, dOut, outPitch / 4, capacityPairs, dCounts);

   hipError_t err = hipGetLastError();
   if (err == hipSuccess)
      err = hipStreamSynchronize(ctx->stream);

   hostCounts.resize(nBuffers);

   if (err == hipSuccess)
      err = hipMemcpy(hostCounts.data(), dCounts, cntBytes, hipMemcpyDeviceToHost);

   if (err == hipSuccess && location == NFCGPU_LOC_HOST)
   {
      err = hipMemcpy(out, dOut, outBytes, hipMemcpyDeviceToHost);
      std::memcpy(counts, hostCounts.data(), cntBytes);
   }

   if (scratch)
      (void)hipFree(scratch);

   if (err != hipSuccess)
      return fail(ctx, NFCGPU_EHIP, "adaptive resampler", err);

   for (uint32_t b = 0; b < nBuffers; b++)
   {
      if (hostCounts[b] > capacityPairs)
         return fail(ctx, NFCGPU_EOVERFLOW, "resampler output capacity exceeded: raise capacity_pairs");
   }

   return NFCGPU_OK;
}

/* The same for rows of any sample layout (nfc_sample.hpp). Float magnitude rows are the call above; the others take the kernels of
 * nfc_resample.hip, which form the loader's magnitude of a sample while they stage it. Host rows are staged as they are. */
int nfcgpu_resample_radio_fmt(nfcgpu_ctx *ctx, const void *in, uint64_t inPitch, uint32_t nBuffers, uint32_t n, uint32_t stride, uint32_t format,
                              float *out, uint64_t outPitch, uint32_t capacityPairs, uint32_t *counts, uint32_t location)
{
   SETTLE_FIRST(ctx);

   if (!ctx)
      return NFCGPU_EINVAL;
   if ((stride != 1 && stride != 2) || (format != NFCGPU_FMT_F32 && format != NFCGPU_FMT_I16))
      return fail(ctx, NFCGPU_EINVAL, "resampler: stride is not 1 or 2, or the format is unknown");

   const uint32_t layout = stride | (format == NFCGPU_FMT_I16 ? NFC_SAMPLE_I16 : 0u);
   const uint32_t sampleBytes = nfc_sample_bytes(layout);

   /* (float magnitude rows: everything but the alignment of `in`, which that call leaves to its caller, is refused there as it is) */
   if (((uintptr_t)in % sampleBytes) != 0 || (layout != 1u && (inPitch % sampleBytes) != 0))
      return fail(ctx, NFCGPU_EINVAL, "resampler: in or in_pitch_bytes is not a multiple of a sample");

   if (layout == 1u)
      return nfcgpu_resample_radio(ctx, (const float *)in, inPitch, nBuffers, n, out, outPitch, capacityPairs, counts, location);

   if (!in || !out || !counts || n < 25 || (outPitch & 7) || ((uintptr_t)out & 7) || inPitch < (uint64_t)n * sampleBytes ||
       outPitch < (uint64_t)capacityPairs * 8 || (location != NFCGPU_LOC_HOST && location != NFCGPU_LOC_DEVICE))
      return NFCGPU_EINVAL;
   if (nBuffers == 0)
      return NFCGPU_OK;

   HIP_TRY(ctx, hipSetDevice(ctx->device));

   NfcResampleArgs A;
   std::memset(&A, 0, sizeof(A));
   A.in = (const uint8_t *)in;
   A.out = out;
   A.counts = counts;
   A.inPitchBytes = inPitch;
   A.outPitchFloats = outPitch / 4;
   A.nBuffers = nBuffers;
   A.n = n;
   A.capacityPairs = capacityPairs;
   A.layout = layout;

   uint8_t *scratch = nullptr;
   std::vector<uint32_t> hostCounts(nBuffers);

   /* what the rows span: the pitch between them, the samples of the last one; out and counts behind it, 8-byte aligned */
   const size_t inBytes = (size_t)inPitch * (nBuffers - 1) + (size_t)n * sampleBytes, inSpace = (inBytes + 7) & ~(size_t)7;
   const size_t outBytes = (size_t)outPitch * nBuffers, cntBytes = (size_t)nBuffers * 4;

   if (location == NFCGPU_LOC_HOST)
   {
      /* one temporary device block: input in its own format, output, counts (this entry point is not on the streaming path) */
      if (hipMalloc((void **)&scratch, inSpace + outBytes + cntBytes) != hipSuccess)
         return fail(ctx, NFCGPU_ENOMEM, "resampler scratch allocation failed");

      hipError_t err = hipMemcpy(scratch, in, inBytes, hipMemcpyHostToDevice);
      if (err != hipSuccess)
      {
         (void)hipFree(scratch);
         return fail(ctx, NFCGPU_EHIP, "hipMemcpy(H2D resampler input)", err);
      }

      A.in = scratch;
      A.out = (float *)(scratch + inSpace);
      A.counts = (uint32_t *)(scratch + inSpace + outBytes);
   }

   const dim3 grid((nBuffers + NfcResampleShape::kLanes - 1) / NfcResampleShape::kLanes), block(NfcResampleShape::kLanes);

   switch (layout)
   {
      case NFC_SAMPLE_I16 | 1u: hipLaunchKernelGGL(nfc_resample_radio_kernel_i16, grid, block, 0, ctx->stream, A); break;
      case NFC_SAMPLE_I16 | 2u: hipLaunchKernelGGL(nfc_resample_radio_kernel_iq_i16, grid, block, 0, ctx->stream, A); break;
      default: hipLaunchKernelGGL(nfc_resample_radio_kernel_iq, grid, block, 0, ctx->stream, A); break;
   }

   hipError_t err = hipGetLastError();
   if (err == hipSuccess)
      err = hipStreamSynchronize(ctx->stream);

   if (err == hipSuccess)
      err = hipMemcpy(hostCounts.data(), A.counts, cntBytes, hipMemcpyDeviceToHost);

   if (err == hipSuccess && location == NFCGPU_LOC_HOST)
   {
      err = hipMemcpy(out, A.out, outBytes, hipMemcpyDeviceToHost);
      std::memcpy(counts, hostCounts.data(), cntBytes);
   }

   if (scratch)
      (void)hipFree(scratch);

   if (err != hipSuccess)
      return fail(ctx, NFCGPU_EHIP, "adaptive resampler", err);

   for (uint32_t b = 0; b < nBuffers; b++)
   {
      if (hostCounts[b] > capacityPairs)
         return fail(ctx, NFCGPU_EOVERFLOW, "resampler output capacity exceeded: raise capacity_pairs");
   }

   return NFCGPU_OK;
}

/* ---- nfcgpu_spectrum: FourierProcessTask::process() (FourierProcessTask.cpp:236-355) for every frame of every buffer ---- */

/* what is wrong with the parameters, or nullptr; *decimation = the D in force */
static const char *spectrum_check(const nfcgpu_spectrum_params *p, uint32_t *decimation)
{
   if (!p)
      return "spectrum: params is NULL";
   if (p->length < 256 || p->length > 4096 || (p->length & (p->length - 1)))
      return "spectrum: length is not a power of two from 256 to 4096";
   if (p->window > NFCGPU_WINDOW_HANN)
      return "spectrum: unknown window";
   if (p->reserved[0] || p->reserved[1] || p->reserved[2])
      return "spectrum: reserved words are not zero";

   /* decimation = int(sampleRate / bandwidth), bandwidth = 10E6 / 16 (FourierProcessTask.cpp:49, :239) */
   uint32_t d = p->decimation ? p->decimation : p->sample_rate / 625000u;
   *decimation = d ? d : 1;
   return nullptr;
}

static uint32_t spectrum_frames(const nfcgpu_spectrum_params *p, uint32_t decimation, uint32_t nPairs)
{
   const uint64_t span = (uint64_t)p->length * decimation;
   if (nPairs < span)
      return 0; /* FourierProcessTask.cpp:242 */
   return p->hop ? (uint32_t)((nPairs - span) / p->hop) + 1 : 1;
}

/* Window (FourierProcessTask.cpp:121-143, the reference's expressions in the reference's types: the sine of "Hamming" is taken of a
 * float and is a float, its square is pow(double, 2)) and twiddles exp(-2 pi i n / L) in double, rounded once. */
static int spectrum_tables(nfcgpu_ctx *ctx, uint32_t length, uint32_t window, const float **dWindow, const float2 **dTwiddle)
{
   for (const nfcgpu_ctx::SpectrumTables &t: ctx->spectrumTables)
   {
      if (t.length == length && t.window == window)
      {
         *dWindow = t.d;
         *dTwiddle = (const float2 *)(t.d + length);
         return NFCGPU_OK;
      }
   }

   const int L = (int)length;
   std::vector<float> host(3 * (size_t)length);

   for (int n = 0; n < L; n++)
   {
      switch (window)
      {
         case NFCGPU_WINDOW_HAMMING:
            host[n] = static_cast<float>(std::pow(std::sin(static_cast<float>(M_PI * n / L)), 2));
            break;
         case NFCGPU_WINDOW_HANN:
            host[n] = static_cast<float>(0.5 * (1.0 - std::cos((2.0 * M_PI * n) / (L - 1))));
            break;
         default:
            host[n] = 1;
            break;
      }

      const double angle = -2.0 * M_PI * (double)n / (double)L;
      host[length + 2 * n] = (float)std::cos(angle);
      host[length + 2 * n + 1] = (float)std::sin(angle);
   }

   nfcgpu_ctx::SpectrumTables t;
   t.length = length;
   t.window = window;

   if (hipMalloc((void **)&t.d, host.size() * sizeof(float)) != hipSuccess)
      return fail(ctx, NFCGPU_ENOMEM, "spectrum tables allocation failed");

   hipError_t err = hipMemcpy(t.d, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice);
   if (err != hipSuccess)
   {
      (void)hipFree(t.d);
      return fail(ctx, NFCGPU_EHIP, "hipMemcpy(H2D spectrum tables)", err);
   }

   ctx->spectrumTables.push_back(t);
   *dWindow = t.d;
   *dTwiddle = (const float2 *)(t.d + length);
   return NFCGPU_OK;
}

void nfcgpu_spectrum_default_params(nfcgpu_spectrum_params *p)
{
   if (!p)
      return;
   std::memset(p, 0, sizeof(*p));
   p->length = 1024;
   p->window = NFCGPU_WINDOW_HAMMING;
   p->sample_rate = 10000000;
}

uint32_t nfcgpu_spectrum_frames(const nfcgpu_spectrum_params *p, uint32_t nPairs)
{
   uint32_t decimation = 1;
   if (spectrum_check(p, &decimation))
      return 0;
   return spectrum_frames(p, decimation, nPairs);
}

int nfcgpu_spectrum(nfcgpu_ctx *ctx, const float *iq, uint64_t inPitch, uint32_t nBuffers, uint32_t nPairs, const nfcgpu_spectrum_params *params,
                    float *out, uint64_t outPitch, uint32_t location)
{
   return nfcgpu_spectrum_fmt(ctx, iq, inPitch, nBuffers, nPairs, params, out, outPitch, location, NFCGPU_FMT_F32);
}

/* (a pair is 8 bytes of float input and 4 of int16; nothing else differs on the host: the rows are staged as they are and the
 * kernel of the format converts while it gathers) */
int nfcgpu_spectrum_fmt(nfcgpu_ctx *ctx, const void *iq, uint64_t inPitch, uint32_t nBuffers, uint32_t nPairs, const nfcgpu_spectrum_params *params,
                        float *out, uint64_t outPitch, uint32_t location, uint32_t format)
{
   SETTLE_FIRST(ctx);

   if (!ctx)
      return NFCGPU_EINVAL;
   if (format != NFCGPU_FMT_F32 && format != NFCGPU_FMT_I16)
      return fail(ctx, NFCGPU_EINVAL, "spectrum: unknown format");

   const bool i16 = format == NFCGPU_FMT_I16;
   const uint32_t pairBytes = i16 ? 4 : 8;

   uint32_t decimation = 1;
   if (const char *why = spectrum_check(params, &decimation))
      return fail(ctx, NFCGPU_EINVAL, why);
   if (!iq || ((uintptr_t)iq & (pairBytes - 1)))
      return fail(ctx, NFCGPU_EINVAL, i16 ? "spectrum: iq is NULL or not 4-byte aligned" : "spectrum: iq is NULL or not 8-byte aligned");
   if (!out || ((uintptr_t)out & 3))
      return fail(ctx, NFCGPU_EINVAL, "spectrum: out is NULL or not 4-byte aligned");
   if (location != NFCGPU_LOC_HOST && location != NFCGPU_LOC_DEVICE)
      return fail(ctx, NFCGPU_EINVAL, "spectrum: unknown location");
   if (inPitch & (pairBytes - 1))
      return fail(ctx, NFCGPU_EINVAL, i16 ? "spectrum: in_pitch_bytes is not a multiple of 4" : "spectrum: in_pitch_bytes is not a multiple of 8");

   const uint32_t L = params->length;
   const uint32_t frames = spectrum_frames(params, decimation, nPairs);
   const uint64_t rowBytes = (uint64_t)frames * L * 4;

   if ((outPitch & 15) || outPitch < rowBytes)
      return fail(ctx, NFCGPU_EINVAL, "spectrum: out_pitch_bytes is not a multiple of 16 or smaller than the frames of a buffer");
   if (nBuffers == 0 || frames == 0)
      return NFCGPU_OK;

   HIP_TRY(ctx, hipSetDevice(ctx->device));

   NfcSpectrumArgs A;
   std::memset(&A, 0, sizeof(A));

   int rc = spectrum_tables(ctx, L, params->window, &A.window, &A.twiddle);
   if (rc)
      return rc;

   uint8_t *scratch = nullptr;
   /* what the buffers span: the pitch between them, the data of the last one */
   const size_t inBytes = (size_t)inPitch * (nBuffers - 1) + (size_t)nPairs * pairBytes, outBytes = (size_t)outPitch * (nBuffers - 1) + (size_t)rowBytes;

   A.iq = (const float2 *)iq;
   A.out = out;

   if (location == NFCGPU_LOC_HOST)
   {
      /* one temporary device block: input, output (this entry point is not on the streaming path) */
      if (hipMalloc((void **)&scratch, inBytes + outBytes) != hipSuccess)
         return fail(ctx, NFCGPU_ENOMEM, "spectrum scratch allocation failed");

      hipError_t err = hipMemcpy(scratch, iq, inBytes, hipMemcpyHostToDevice);
      if (err != hipSuccess)
      {
         (void)hipFree(scratch);
         return fail(ctx, NFCGPU_EHIP, "hipMemcpy(H2D spectrum input)", err);
      }

      A.iq = (const float2 *)scratch;
      A.out = (float *)(scratch + inBytes);
   }

   A.inPitchPairs = inPitch / pairBytes;
   A.outPitchFloats = outPitch / 4;
   A.total = (uint64_t)nBuffers * frames;
   A.frames = frames;
   A.hop = params->hop;
   A.decimation = decimation;

   /* one workgroup per frame; beyond 2^20 workgroups each takes several frames */
   const dim3 grid((uint32_t)(A.total < (1u << 20) ? A.total : (1u << 20)));

#define NFC_SPECTRUM_LAUNCH(L) \
   hipLaunchKernelGGL(i16 ? nfc_spectrum_kernel_i16_##L : nfc_spectrum_kernel_##L, grid, dim3(NfcSpectrumShape<L>::kThreads), 0, ctx->stream, A)

   switch (L)
   {
      case 256: NFC_SPECTRUM_LAUNCH(256); break;
      case 512: NFC_SPECTRUM_LAUNCH(512); break;
      case 1024: NFC_SPECTRUM_LAUNCH(1024); break;
      case 2048: NFC_SPECTRUM_LAUNCH(2048); break;
      default: NFC_SPECTRUM_LAUNCH(4096); break;
   }
#undef NFC_SPECTRUM_LAUNCH

   hipError_t err = hipGetLastError();
   if (err == hipSuccess)
      err = hipStreamSynchronize(ctx->stream);

   if (err == hipSuccess && location == NFCGPU_LOC_HOST)
   {
      /* the frames of every buffer go to the caller's rows; what lies between the rows is the caller's */
      std::vector<uint8_t> back(outBytes);
      err = hipMemcpy(back.data(), A.out, outBytes, hipMemcpyDeviceToHost);
      if (err == hipSuccess)
      {
         for (uint32_t b = 0; b < nBuffers; b++)
            std::memcpy((uint8_t *)out + (size_t)b * outPitch, back.data() + (size_t)b * outPitch, (size_t)rowBytes);
      }
   }

   if (scratch)
      (void)hipFree(scratch);

   if (err != hipSuccess)
      return fail(ctx, NFCGPU_EHIP, "spectrum", err);

   return NFCGPU_OK;
}

/* ---- nfcgpu_record: the recording pass (SignalStorageTask.cpp:493-523, RecordDevice.cpp:313-348) and the levels of
 * RadioDeviceTask::processQueue (RadioDeviceTask.cpp:547-680) in one read of every buffer ---- */

static_assert(sizeof(nfcgpu_record_levels) == sizeof(NfcRecordPartial) && sizeof(NfcRecordPartial) == 16, "a levels record is 16 bytes");

/* the powers of w0 = 1 - 0.001f the kernels weight with, in double, rounded once */
static void record_weights(NfcRecordWeights &w, uint32_t n)
{
   const float w1 = 0.001f, w0 = 1.0f - w1;
   const uint64_t quads = ((uint64_t)n + 3) / 4;
   const uint64_t lastQuads = quads - (quads - 1) / NfcRecordShape::kSegmentQuads * NfcRecordShape::kSegmentQuads;

   w.w1 = w1;
   w.w64 = (float)std::pow((double)w0, 64.0);
   w.segment = (float)std::pow((double)w0, (double)NfcRecordShape::kSegmentQuads);
   w.last = (float)std::pow((double)w0, (double)lastQuads);
   w.unpad = (float)std::pow((double)w0, -(double)(NfcRecordShape::kSegmentQuads - lastQuads));
   for (uint32_t i = 0; i < NfcRecordShape::kWaves; i++)
      w.wave[i] = (float)std::pow((double)w0, (double)(NfcRecordShape::kWaveQuads * (NfcRecordShape::kWaves - 1 - i)));
   for (uint32_t i = 0; i < 64; i++)
      w.lane[i] = (float)std::pow((double)w0, (double)(63 - i));
}

int nfcgpu_record(nfcgpu_ctx *ctx, const float *in, uint64_t inPitch, uint32_t nBuffers, uint32_t n, uint32_t stride, uint32_t mode, int16_t *out,
                  uint64_t outPitch, nfcgpu_record_levels *levels, uint32_t location)
{
   SETTLE_FIRST(ctx);

   if (!ctx)
      return NFCGPU_EINVAL;
   if (stride != 1 && stride != 2)
      return fail(ctx, NFCGPU_EINVAL, "record: stride is neither 1 nor 2");
   if (mode != NFCGPU_RECORD_SAME && mode != NFCGPU_RECORD_MAGNITUDE)
      return fail(ctx, NFCGPU_EINVAL, "record: unknown mode");
   if (mode == NFCGPU_RECORD_MAGNITUDE && stride != 2)
      return fail(ctx, NFCGPU_EINVAL, "record: mode NFCGPU_RECORD_MAGNITUDE needs stride 2");
   if (location != NFCGPU_LOC_HOST && location != NFCGPU_LOC_DEVICE)
      return fail(ctx, NFCGPU_EINVAL, "record: unknown location");

   const uint32_t channels = (stride == 2 && mode == NFCGPU_RECORD_SAME) ? 2 : 1;
   const uint64_t inSample = 4 * stride, outSample = 2 * channels;
   const uint64_t rowBytes = (uint64_t)n * outSample;

   if (!in || ((uintptr_t)in % inSample))
      return fail(ctx, NFCGPU_EINVAL, "record: in is NULL or not aligned to a sample (4 * stride bytes)");
   if (!out || ((uintptr_t)out % outSample))
      return fail(ctx, NFCGPU_EINVAL, "record: out is NULL or not aligned to a PCM sample (2 * channels bytes)");
   if (levels && ((uintptr_t)levels & 3))
      return fail(ctx, NFCGPU_EINVAL, "record: levels is not 4-byte aligned");
   if (inPitch % inSample)
      return fail(ctx, NFCGPU_EINVAL, "record: in_pitch_bytes is not a multiple of a sample (4 * stride bytes)");
   if ((outPitch % outSample) || outPitch < rowBytes)
      return fail(ctx, NFCGPU_EINVAL, "record: out_pitch_bytes is not a multiple of a PCM sample (2 * channels bytes) or smaller than a row");
   if (nBuffers == 0)
      return NFCGPU_OK;

   HIP_TRY(ctx, hipSetDevice(ctx->device));

   const size_t levelBytes = levels ? (size_t)nBuffers * sizeof(nfcgpu_record_levels) : 0;

   if (n == 0)
   {
      if (levels && location == NFCGPU_LOC_HOST)
         std::memset(levels, 0, levelBytes);
      else if (levels)
      {
         HIP_TRY(ctx, hipMemsetAsync(levels, 0, levelBytes, ctx->stream));
         HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
      }
      return NFCGPU_OK;
   }

   NfcRecordArgs A;
   std::memset(&A, 0, sizeof(A));

   A.nSegments = (uint32_t)(((uint64_t)n + NfcRecordShape::kSegmentSamples - 1) / NfcRecordShape::kSegmentSamples);
   A.total = (uint64_t)nBuffers * A.nSegments;
   A.n = n;
   A.nBuffers = nBuffers;
   A.inPitch = inPitch;
   A.outPitch = outPitch;
   record_weights(A.w, n);

   if (levels)
   {
      const size_t need = (size_t)A.total * sizeof(NfcRecordPartial);

      if (need > ctx->recordPartialsBytes)
      {
         if (ctx->recordPartials)
            (void)hipFree(ctx->recordPartials);
         ctx->recordPartials = nullptr;
         ctx->recordPartialsBytes = 0;
         if (hipMalloc(&ctx->recordPartials, need) != hipSuccess)
            return fail(ctx, NFCGPU_ENOMEM, "record: scratch for the levels could not be allocated");
         ctx->recordPartialsBytes = need;
      }

      A.partials = (NfcRecordPartial *)ctx->recordPartials;
   }

   uint8_t *scratch = nullptr;
   /* what the buffers span: the pitch between them, the data of the last one */
   const size_t inBytes = (size_t)inPitch * (nBuffers - 1) + (size_t)n * inSample, outBytes = (size_t)outPitch * (nBuffers - 1) + (size_t)rowBytes;
   /* (the copy of `out` lies as `out` does within 16 bytes, so the kernel packs its stores as it would in place) */
   const size_t inRoom = (inBytes + 15) & ~(size_t)15, outShift = (uintptr_t)out & 15, outRoom = (outShift + outBytes + 15) & ~(size_t)15;

   A.in = in;
   A.out = out;
   A.levels = (NfcRecordPartial *)levels;

   if (location == NFCGPU_LOC_HOST)
   {
      /* one temporary device block: input, output, levels (this entry point is not on the streaming path) */
      if (hipMalloc((void **)&scratch, inRoom + outRoom + levelBytes) != hipSuccess)
         return fail(ctx, NFCGPU_ENOMEM, "record: scratch allocation failed");

      hipError_t err = hipMemcpy(scratch, in, inBytes, hipMemcpyHostToDevice);
      if (err != hipSuccess)
      {
         (void)hipFree(scratch);
         return fail(ctx, NFCGPU_EHIP, "hipMemcpy(H2D record input)", err);
      }

      A.in = (const float *)scratch;
      A.out = (int16_t *)(scratch + inRoom + outShift);
      A.levels = levels ? (NfcRecordPartial *)(scratch + inRoom + outRoom) : nullptr;
   }

   /* one workgroup per segment; beyond 2^20 workgroups each takes several */
   const dim3 grid((uint32_t)(A.total < (1u << 20) ? A.total : (1u << 20))), block(NfcRecordShape::kThreads);

   if (stride == 1)
   {
      if (levels)
         hipLaunchKernelGGL(nfc_record_kernel_mono_levels, grid, block, 0, ctx->stream, A);
      else
         hipLaunchKernelGGL(nfc_record_kernel_mono, grid, block, 0, ctx->stream, A);
   }
   else if (mode == NFCGPU_RECORD_SAME)
   {
      if (levels)
         hipLaunchKernelGGL(nfc_record_kernel_iq_levels, grid, block, 0, ctx->stream, A);
      else
         hipLaunchKernelGGL(nfc_record_kernel_iq, grid, block, 0, ctx->stream, A);
   }
   else
   {
      if (levels)
         hipLaunchKernelGGL(nfc_record_kernel_magnitude_levels, grid, block, 0, ctx->stream, A);
      else
         hipLaunchKernelGGL(nfc_record_kernel_magnitude, grid, block, 0, ctx->stream, A);
   }

   hipError_t err = hipGetLastError();

   if (err == hipSuccess && levels)
   {
      hipLaunchKernelGGL(nfc_record_finish_kernel, dim3(nBuffers < 65536u ? nBuffers : 65536u), dim3(64), 0, ctx->stream, A);
      err = hipGetLastError();
   }

   if (err == hipSuccess)
      err = hipStreamSynchronize(ctx->stream);

   if (err == hipSuccess && location == NFCGPU_LOC_HOST)
   {
      /* the PCM of every buffer goes to the caller's rows; what lies between the rows is the caller's */
      std::vector<uint8_t> back(outBytes + levelBytes);
      err = hipMemcpy(back.data(), A.out, outBytes, hipMemcpyDeviceToHost);
      if (err == hipSuccess && levels)
         err = hipMemcpy(back.data() + outBytes, A.levels, levelBytes, hipMemcpyDeviceToHost);
      if (err == hipSuccess)
      {
         for (uint32_t b = 0; b < nBuffers; b++)
            std::memcpy((uint8_t *)out + (size_t)b * outPitch, back.data() + (size_t)b * outPitch, (size_t)rowBytes);
         if (levels)
            std::memcpy(levels, back.data() + outBytes, levelBytes);
      }
   }

   if (scratch)
      (void)hipFree(scratch);

   if (err != hipSuccess)
      return fail(ctx, NFCGPU_EHIP, "record", err);

   return NFCGPU_OK;
}

/* ---- nfcgpu_signal_tap: the front end's per-sample signals (NfcDecoderStatus::nextSample with setEnableDebug(true),
 * NfcTech.cpp:28-105) for buffers wherever they lie, cut in time (nfc_tap.hpp) ---- */

static_assert(sizeof(nfcgpu_tap_state) == sizeof(NfcTapRecord) && sizeof(NfcTapRecord) == 32 && sizeof(NfcTapState) == 24, "a tap state is 32 bytes, 24 of them used");
static_assert(NFCGPU_TAP_VALUE == NFC_TAP_VALUE && NFCGPU_TAP_FILTERED == NFC_TAP_FILTERED && NFCGPU_TAP_DEVIATION == NFC_TAP_DEVIATION &&
              NFCGPU_TAP_AVERAGE == NFC_TAP_AVERAGE && NFCGPU_TAP_ENVELOPE == NFC_TAP_ENVELOPE && NFCGPU_TAP_DEPTH == NFC_TAP_DEPTH, "the planes of the header");

/* The library's choice of chunk and warm-up (the section on the tap). Warm-up: 4096 samples at 10 MS/s, as many time
 * constants of the slowest recurrence (the average, 1 / meanW1 samples) at any rate. Chunk: what cuts the call into about kTapWalkers
 * walkers, a wave for every SIMD of the chip, and no shorter than kTapMinChunk; a call of many buffers, which fills waves whatever
 * the chunk, takes chunks of at least twice the warm-up; never more than a buffer. */
constexpr uint64_t kTapWalkers = 65536;
constexpr uint64_t kTapMinChunk = 256;
constexpr uint32_t kTapManyBuffers = 1024;
constexpr uint32_t kTapMaxChunk = 0xFFFFFFC0u;

static uint32_t tap_default_warm(uint32_t sampleRate)
{
   uint64_t w = ((uint64_t)sampleRate * 4096u + 9999999u) / 10000000u;
   w = (w + 63u) & ~(uint64_t)63;
   return (uint32_t)(w < 64u ? 64u : (w > 8192u ? 8192u : w));
}

static uint32_t tap_default_chunk(uint32_t nBuffers, uint32_t n, uint32_t warm)
{
   uint64_t c = (uint64_t)nBuffers * n / kTapWalkers;

   if (c < kTapMinChunk)
      c = kTapMinChunk;
   if (nBuffers >= kTapManyBuffers && c < 2ull * warm)
      c = 2ull * warm;

   const uint64_t whole = ((uint64_t)n + 63u) & ~(uint64_t)63;

   if (c > whole)
      c = whole;
   c = (c + 63u) & ~(uint64_t)63;
   return c > kTapMaxChunk ? kTapMaxChunk : (uint32_t)c;
}

void nfcgpu_tap_state_init(nfcgpu_tap_state *s)
{
   if (!s)
      return;
   std::memset(s, 0, sizeof(*s));
   s->clock = 0xFFFFFFFFu;
}

/* What nfcgpu_signal_tap and nfcgpu_signal_tap_reduce refuse alike, in the order the tap checks it: the parameters and the input
 * ahead of the tap's own checks of its planes, the states and the rate behind them. */
static int tap_check_input(nfcgpu_ctx *ctx, const void *in, uint64_t inPitch, uint32_t nBuffers, uint32_t n, uint32_t stride, uint32_t format,
                           const nfcgpu_tap_params *params, uint32_t location)
{
   if (!params)
      return fail(ctx, NFCGPU_EINVAL, "tap: params is NULL");
   if (params->channels == 0 || (params->channels & ~NFC_TAP_ALL))
      return fail(ctx, NFCGPU_EINVAL, "tap: channels is 0 or has bits that are no NFCGPU_TAP_* channel");
   if (params->reserved[0] | params->reserved[1] | params->reserved[2] | params->reserved[3])
      return fail(ctx, NFCGPU_EINVAL, "tap: reserved fields of params are not zero");
   if (stride != 1 && stride != 2)
      return fail(ctx, NFCGPU_EINVAL, "tap: stride is neither 1 nor 2");
   if (format != NFCGPU_FMT_F32 && format != NFCGPU_FMT_I16)
      return fail(ctx, NFCGPU_EINVAL, "tap: unknown format");
   if (location != NFCGPU_LOC_HOST && location != NFCGPU_LOC_DEVICE)
      return fail(ctx, NFCGPU_EINVAL, "tap: unknown location");
   if (params->chunk_samples % 64u)
      return fail(ctx, NFCGPU_EINVAL, "tap: chunk_samples is not a multiple of 64");

   const uint64_t sampleBytes = nfc_sample_bytes(stride | (format == NFCGPU_FMT_I16 ? NFC_SAMPLE_I16 : 0u));

   if (!in || ((uintptr_t)in % sampleBytes))
      return fail(ctx, NFCGPU_EINVAL, "tap: in is NULL or not aligned to a sample");
   if ((inPitch % sampleBytes) || (nBuffers > 1 && inPitch < (uint64_t)n * sampleBytes))
      return fail(ctx, NFCGPU_EINVAL, "tap: in_pitch_bytes is not a multiple of a sample or smaller than a row");

   return NFCGPU_OK;
}

static int tap_check_states_and_rate(nfcgpu_ctx *ctx, const nfcgpu_tap_params *params, const nfcgpu_tap_state *stateIn, const nfcgpu_tap_state *stateOut, NfcConfig &cfg)
{
   if (((uintptr_t)stateIn & 3) || ((uintptr_t)stateOut & 3))
      return fail(ctx, NFCGPU_EINVAL, "tap: state_in or state_out is not 4-byte aligned");
   if (params->sample_rate == 0)
      return fail(ctx, NFCGPU_EINVAL, "tap: sample rate must be non-zero");

   NfcHostParams hp;
   hp.sampleRate = params->sample_rate;
   if (!nfc_build_config(hp, cfg))
      return fail(ctx, NFCGPU_ERATE, "tap: sample rate not decodable with the fixed history depth");

   return NFCGPU_OK;
}

int nfcgpu_signal_tap(nfcgpu_ctx *ctx, const void *in, uint64_t inPitch, uint32_t nBuffers, uint32_t n, uint32_t stride, uint32_t format,
                      const nfcgpu_tap_params *params, const nfcgpu_tap_state *stateIn, float *out, uint64_t outPitch, uint64_t planePitch,
                      nfcgpu_tap_state *stateOut, nfcgpu_tap_report *report, uint32_t location)
{
   SETTLE_FIRST(ctx);

   if (!ctx)
      return NFCGPU_EINVAL;

   int rc = tap_check_input(ctx, in, inPitch, nBuffers, n, stride, format, params, location);
   if (rc)
      return rc;

   const uint32_t layout = stride | (format == NFCGPU_FMT_I16 ? NFC_SAMPLE_I16 : 0u);
   const uint64_t sampleBytes = nfc_sample_bytes(layout);
   const uint32_t planes = nfc_tap_planes(params->channels);
   const uint64_t planeBytes = (uint64_t)n * 4u;

   if (!out || ((uintptr_t)out & 3))
      return fail(ctx, NFCGPU_EINVAL, "tap: out is NULL or not 4-byte aligned");
   if ((planePitch % 16u) || planePitch < planeBytes)
      return fail(ctx, NFCGPU_EINVAL, "tap: plane_pitch_bytes is not a multiple of 16 or smaller than a plane");
   if ((outPitch % 16u) || (nBuffers > 1 && outPitch < (uint64_t)(planes - 1) * planePitch + planeBytes))
      return fail(ctx, NFCGPU_EINVAL, "tap: out_pitch_bytes is not a multiple of 16 or smaller than the planes of a buffer");

   NfcConfig cfg;

   rc = tap_check_states_and_rate(ctx, params, stateIn, stateOut, cfg);
   if (rc)
      return rc;

   if (report)
      std::memset(report, 0, sizeof(*report));

   HIP_TRY(ctx, hipSetDevice(ctx->device));

   const size_t stateBytes = (size_t)nBuffers * sizeof(NfcTapRecord);

   if (nBuffers == 0)
      return NFCGPU_OK;

   if (n == 0)
   {
      /* nothing walked: state_out is state_in */
      if (stateOut)
      {
         std::vector<nfcgpu_tap_state> fresh;

         if (!stateIn)
         {
            fresh.resize(nBuffers);
            for (nfcgpu_tap_state &s: fresh)
               nfcgpu_tap_state_init(&s);
         }

         if (location == NFCGPU_LOC_HOST)
            std::memmove(stateOut, stateIn ? stateIn : fresh.data(), stateBytes);
         else
         {
            HIP_TRY(ctx, hipMemcpyAsync(stateOut, stateIn ? stateIn : fresh.data(), stateBytes, stateIn ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream));
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
         }
      }
      return NFCGPU_OK;
   }

   NfcTapArgs A;
   std::memset(&A, 0, sizeof(A));

   A.warm = params->chunk_samples ? params->warm_samples : tap_default_warm(params->sample_rate);
   A.chunk = params->chunk_samples ? params->chunk_samples : tap_default_chunk(nBuffers, n, A.warm);
   A.chunksPerBuffer = (uint32_t)(((uint64_t)n + A.chunk - 1) / A.chunk);
   A.n = n;
   A.nBuffers = nBuffers;
   A.layout = layout;
   A.mask = params->channels;
   A.walkers = (uint64_t)nBuffers * A.chunksPerBuffer;

   if (A.walkers > 0xFFFFFFFFull)
      return fail(ctx, NFCGPU_EINVAL, "tap: more than 2^32 - 1 chunks (chunk_samples is too small for this much input)");

   const uint32_t C = A.chunksPerBuffer;
   const uint64_t reach = (uint64_t)(C - 1) * A.chunk; /* where the last chunk of a buffer begins: no warm-up is longer */
   const uint64_t longest = (A.warm < reach ? A.warm : reach) + (A.chunk < n ? A.chunk : n);

   A.tiles = (uint32_t)((longest + NfcTapShape::kTile - 1) / NfcTapShape::kTile);

   /* scratch: starts, ends, list, frontier, next, count */
   const size_t statesAt = 0, statesBytes = ((size_t)A.walkers * sizeof(NfcTapState) + 15) & ~(size_t)15;
   const size_t wordsBytes = ((size_t)nBuffers * 4 + 15) & ~(size_t)15;
   const size_t listAt = statesAt + 2 * statesBytes, frontierAt = listAt + wordsBytes, nextAt = frontierAt + wordsBytes, countAt = nextAt + wordsBytes;
   const size_t need = countAt + 16;

   if (need > ctx->tapScratchBytes)
   {
      if (ctx->tapScratch)
         (void)hipFree(ctx->tapScratch);
      ctx->tapScratch = nullptr;
      ctx->tapScratchBytes = 0;
      if (hipMalloc(&ctx->tapScratch, need) != hipSuccess)
         return fail(ctx, NFCGPU_ENOMEM, "tap: scratch for the walkers' states could not be allocated");
      ctx->tapScratchBytes = need;
   }

   if (!ctx->tapCount && hipHostMalloc((void **)&ctx->tapCount, 16, hipHostMallocDefault) != hipSuccess)
   {
      ctx->tapCount = nullptr;
      return fail(ctx, NFCGPU_ENOMEM, "tap: pinned word for the rounds could not be allocated");
   }

   uint8_t *scratch = (uint8_t *)ctx->tapScratch;

   A.starts = (NfcTapState *)(scratch + statesAt);
   A.ends = (NfcTapState *)(scratch + statesAt + statesBytes);
   A.listOut = (uint32_t *)(scratch + listAt);
   A.frontier = (uint32_t *)(scratch + frontierAt);
   A.next = (uint32_t *)(scratch + nextAt);
   A.count = (uint32_t *)(scratch + countAt);

   A.in = (const uint8_t *)in;
   A.out = out;
   A.inPitch = inPitch;
   A.outPitch = outPitch;
   A.planePitch = planePitch;
   A.stateIn = (const NfcTapRecord *)stateIn;
   A.stateOut = (NfcTapRecord *)stateOut;

   /* host memory goes through the staging slots: rows and state_in up through one, planes and state_out back through the other */
   nfcgpu_ctx::StageSlot *up = nullptr, *down = nullptr;

   struct Release
   {
      nfcgpu_ctx *ctx;
      nfcgpu_ctx::StageSlot **up, **down;
      ~Release()
      {
         if (*up)
            stage_release(ctx, *up);
         if (*down)
            stage_release(ctx, *down);
      }
   } release {ctx, &up, &down};

   const size_t rowBytes = (size_t)n * sampleBytes;
   size_t downPlane = 0, downPitch = 0, downStates = 0;

   ctx->inflight = true;

   if (location == NFCGPU_LOC_HOST)
   {
      const size_t upPitch = (rowBytes + 255) & ~(size_t)255, upStates = upPitch * nBuffers;

      int rc = stage_acquire(ctx, upStates + stateBytes, &up);
      if (rc)
         return rc;

      for (uint32_t b = 0; b < nBuffers; b++)
         std::memcpy(up->h + (size_t)b * upPitch, (const uint8_t *)in + (size_t)b * inPitch, rowBytes);
      if (stateIn)
         std::memcpy(up->h + upStates, stateIn, stateBytes);

      HIP_TRY(ctx, hipMemcpyAsync(up->d, up->h, upStates + (stateIn ? stateBytes : 0), hipMemcpyHostToDevice, ctx->stream));

      downPlane = ((size_t)planeBytes + 255) & ~(size_t)255;
      downPitch = downPlane * planes;
      downStates = downPitch * nBuffers;

      rc = stage_acquire(ctx, downStates + stateBytes, &down);
      if (rc)
         return rc;

      A.in = up->d;
      A.inPitch = upPitch;
      A.stateIn = stateIn ? (const NfcTapRecord *)(up->d + upStates) : nullptr;
      A.out = (float *)down->d;
      A.outPitch = downPitch;
      A.planePitch = downPlane;
      A.stateOut = stateOut ? (NfcTapRecord *)(down->d + downStates) : nullptr;
   }

   const size_t lds = (size_t)(1 + planes) * NfcTapShape::kPlaneFloats * sizeof(float);
   (void)lds; /* (the emulated test build's launches take no LDS) */
   auto walk_grid = [](uint64_t walkers) {
      const uint64_t groups = (walkers + NfcTapShape::kWalkers - 1) / NfcTapShape::kWalkers;
      return dim3((uint32_t)(groups < (1u << 20) ? groups : (1u << 20)));
   };
   const uint64_t seamBlocks = (A.walkers + 255) / 256, listBlocks = ((uint64_t)nBuffers + 255) / 256;
   const dim3 seamGrid((uint32_t)(seamBlocks < 65536 ? seamBlocks : 65536)), listGrid((uint32_t)(listBlocks < 65536 ? listBlocks : 65536));

   /* the first walk: every chunk */
   hipLaunchKernelGGL(nfc_tap_walk_kernel, walk_grid(A.walkers), dim3(NfcTapShape::kWalkers), lds, ctx->stream, A, cfg);
   HIP_TRY(ctx, hipGetLastError());

   uint32_t rounds = 0;
   uint64_t rewalked = 0;

   if (C > 1)
   {
      /* nothing is true yet but the first chunks (a frontier of 0 and of 1 are the same: chunk 0 is never looked at), none found to differ */
      HIP_TRY(ctx, hipMemsetAsync(A.frontier, 0, wordsBytes, ctx->stream));
      HIP_TRY(ctx, hipMemsetAsync(A.next, 0xFF, wordsBytes, ctx->stream));

      NfcTapArgs R = A;
      R.list = A.listOut;
      R.tiles = ((A.chunk < n ? A.chunk : n) + NfcTapShape::kTile - 1) / NfcTapShape::kTile;

      for (;;)
      {
         HIP_TRY(ctx, hipMemsetAsync(A.count, 0, 16, ctx->stream));
         hipLaunchKernelGGL(nfc_tap_seam_kernel, seamGrid, dim3(256), 0, ctx->stream, A);
         HIP_TRY(ctx, hipGetLastError());
         hipLaunchKernelGGL(nfc_tap_list_kernel, listGrid, dim3(256), 0, ctx->stream, A);
         HIP_TRY(ctx, hipGetLastError());
         HIP_TRY(ctx, hipMemcpyAsync(ctx->tapCount, A.count, 4, hipMemcpyDeviceToHost, ctx->stream));
         HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));

         const uint32_t listed = ctx->tapCount[0];

         if (listed == 0)
            break;

         /* (every round moves the frontier of every buffer it lists by a chunk at least: C - 1 rounds at the most) */
         if (rounds >= C - 1 || listed > nBuffers)
            return fail(ctx, NFCGPU_EHIP, "tap: the rounds of second walks did not end (internal error)");

         rounds++;
         rewalked += listed;
         R.walkers = listed;
         hipLaunchKernelGGL(nfc_tap_walk_kernel, walk_grid(listed), dim3(NfcTapShape::kWalkers), lds, ctx->stream, R, cfg);
         HIP_TRY(ctx, hipGetLastError());
      }
   }

   if (A.stateOut)
   {
      hipLaunchKernelGGL(nfc_tap_finish_kernel, listGrid, dim3(256), 0, ctx->stream, A);
      HIP_TRY(ctx, hipGetLastError());
   }

   if (location == NFCGPU_LOC_HOST)
   {
      HIP_TRY(ctx, hipMemcpyAsync(down->h, down->d, downStates + (stateOut ? stateBytes : 0), hipMemcpyDeviceToHost, ctx->stream));
      HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));

      /* the planes go to the caller's rows; what lies between them is the caller's */
      for (uint32_t b = 0; b < nBuffers; b++)
         for (uint32_t k = 0; k < planes; k++)
            std::memcpy((uint8_t *)out + (size_t)b * outPitch + (size_t)k * planePitch, down->h + (size_t)b * downPitch + (size_t)k * downPlane, (size_t)planeBytes);
      if (stateOut)
         std::memcpy(stateOut, down->h + downStates, stateBytes);
   }
   else
      HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));

   if (report)
   {
      report->chunks = (uint32_t)A.walkers;
      report->rounds = rounds;
      report->rewalked_chunks = (uint32_t)(rewalked > 0xFFFFFFFFull ? 0xFFFFFFFFull : rewalked);
   }

   return NFCGPU_OK;
}

/* ---- nfcgpu_signal_tap_reduce: the tap over slabs of whole buffers into planes the context owns, every slab reduced over the
 * ranges that lie in it (nfc_tap_reduce.hpp) ---- */

static_assert(sizeof(nfcgpu_tap_range) == sizeof(NfcTapRange) && sizeof(NfcTapRange) == 16, "a tap range is 16 bytes");
static_assert(sizeof(nfcgpu_tap_stat) == sizeof(NfcTapStat) && sizeof(NfcTapStat) == 32 && sizeof(NfcTapPartial) == 32, "a tap record and a partial are 32 bytes");

constexpr uint64_t kTapReduceBlocks = 8192;          /* of four waves: some waves per SIMD, the rest of the units by stride */

int nfcgpu_signal_tap_reduce(nfcgpu_ctx *ctx, const void *in, uint64_t inPitch, uint32_t nBuffers, uint32_t n, uint32_t stride, uint32_t format,
                             const nfcgpu_tap_params *tap, const nfcgpu_tap_reduce_params *reduce, const nfcgpu_tap_state *stateIn,
                             const nfcgpu_tap_range *ranges, uint32_t nRanges, nfcgpu_tap_stat *out, nfcgpu_tap_state *stateOut,
                             nfcgpu_tap_report *report, uint32_t location)
{
   SETTLE_FIRST(ctx);

   if (!ctx)
      return NFCGPU_EINVAL;

   int rc = tap_check_input(ctx, in, inPitch, nBuffers, n, stride, format, tap, location);
   if (rc)
      return rc;

   if (!reduce)
      return fail(ctx, NFCGPU_EINVAL, "tap reduce: reduce is NULL");
   if (reduce->reserved0 | reduce->reserved[0] | reduce->reserved[1] | reduce->reserved[2] | reduce->reserved[3])
      return fail(ctx, NFCGPU_EINVAL, "tap reduce: reserved fields of reduce are not zero");
   if (!ranges && nRanges != 0)
      return fail(ctx, NFCGPU_EINVAL, "tap reduce: ranges is NULL and n_ranges is not 0");
   if (!ranges && reduce->bin_samples == 0)
      return fail(ctx, NFCGPU_EINVAL, "tap reduce: neither ranges nor bin_samples");
   if (((uintptr_t)out & 3) || ((uintptr_t)ranges & 3))
      return fail(ctx, NFCGPU_EINVAL, "tap reduce: out or ranges is not 4-byte aligned");

   NfcConfig cfg;

   rc = tap_check_states_and_rate(ctx, tap, stateIn, stateOut, cfg);
   if (rc)
      return rc;

   const bool host = location == NFCGPU_LOC_HOST;
   const uint32_t K = nfc_tap_planes(tap->channels);
   const uint32_t bin = reduce->bin_samples;
   const uint32_t bins = ranges ? 0u : (uint32_t)(((uint64_t)n + bin - 1) / bin);
   const uint64_t nRecordRanges = ranges ? (uint64_t)nRanges : (uint64_t)nBuffers * bins;

   if (nRecordRanges * K > 0xFFFFFFFFull)
      return fail(ctx, NFCGPU_EINVAL, "tap reduce: more than 2^32 - 1 records");
   if (nRecordRanges && !out)
      return fail(ctx, NFCGPU_EINVAL, "tap reduce: out is NULL");

   auto range_ok = [&](const NfcTapRange &g) { return g.buffer < nBuffers && g.reserved == 0 && g.first <= n && g.count <= n - g.first; };

   if (host && nBuffers)
   {
      for (uint32_t r = 0; r < nRanges; r++)
      {
         if (!range_ok(reinterpret_cast<const NfcTapRange *>(ranges)[r]))
         {
            const std::string what = "tap reduce: range " + std::to_string(r) + " is not inside the buffers (buffer, first + count) or its reserved field is not zero";
            return fail(ctx, NFCGPU_EINVAL, what.c_str());
         }
      }
   }

   if (report)
      std::memset(report, 0, sizeof(*report));

   HIP_TRY(ctx, hipSetDevice(ctx->device));

   if (nBuffers == 0)
      return NFCGPU_OK;

   const size_t records = (size_t)(nRecordRanges * K);
   const size_t stateBytes = (size_t)nBuffers * sizeof(NfcTapRecord);
   const size_t rangesBytes = (size_t)nRanges * sizeof(NfcTapRange);
   const uint32_t layout = stride | (format == NFCGPU_FMT_I16 ? NFC_SAMPLE_I16 : 0u);
   const size_t rowBytes = (size_t)n * nfc_sample_bytes(layout);
   auto round16 = [](size_t v) { return (v + 15) & ~(size_t)15; };

   /* the ranges as the host sees them, for the plan alone: device ranges are copied down, the kernels check them where they lie */
   std::vector<NfcTapRange> copied;
   const NfcTapRange *seen = reinterpret_cast<const NfcTapRange *>(ranges);

   if (!host && nRanges)
   {
      copied.resize(nRanges);
      HIP_TRY(ctx, hipMemcpyAsync(copied.data(), ranges, rangesBytes, hipMemcpyDeviceToHost, ctx->stream));
      HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
      seen = copied.data();
   }

   /* the plan: the ranges by buffer (what is in no buffer behind them all), the segments ahead of each, every segment by name */
   std::vector<uint32_t> order(nRanges), keys(nRanges);
   std::vector<uint64_t> prefix((size_t)nRanges + 1, 0);
   std::vector<NfcTapSegment> table;

   if (ranges)
   {
      auto key = [&](uint32_t r) { return seen[r].buffer < nBuffers ? seen[r].buffer : nBuffers; };

      for (uint32_t r = 0; r < nRanges; r++)
         order[r] = r;
      if (!std::is_sorted(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return key(a) < key(b); }))
         std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return key(a) < key(b); });
      for (uint32_t o = 0; o < nRanges; o++)
      {
         keys[o] = key(order[o]);
         prefix[o + 1] = prefix[o] + (range_ok(seen[order[o]]) ? nfc_tap_segments(seen[order[o]].count) : 0u);
      }

      table.reserve((size_t)prefix[nRanges]);
      for (uint32_t o = 0; o < nRanges; o++)
         for (uint32_t s = 0; s < (uint32_t)(prefix[o + 1] - prefix[o]); s++)
            table.push_back(NfcTapSegment {order[o], s});
   }

   const uint32_t segsPerBin = ranges ? 0u : nfc_tap_segments(bin < n ? bin : n);

   /* the items and the segments of the slab b0 ... b1 - 1 */
   auto slab_plan = [&](uint32_t b0, uint32_t b1, uint64_t &firstItem, uint64_t &items, uint64_t &segments) {
      if (!ranges)
      {
         firstItem = (uint64_t)b0 * bins;
         items = (uint64_t)(b1 - b0) * bins;
         segments = items * segsPerBin;
         return;
      }
      const uint64_t o0 = std::lower_bound(keys.begin(), keys.end(), b0) - keys.begin();
      const uint64_t o1 = b1 == nBuffers ? nRanges : (uint64_t)(std::lower_bound(keys.begin(), keys.end(), b1) - keys.begin());
      firstItem = o0;
      items = o1 - o0;
      segments = prefix[o1] - prefix[o0];
   };

   const uint64_t planePitch = std::max<uint64_t>(((uint64_t)n * 4u + 255) & ~(uint64_t)255, 256);
   const uint64_t bufferPitch = planePitch * K;

   /* scratch_bytes == 0: every slab pays the tap's rounds anew, so all the planes at once where three quarters of
    * the device memory that is free (this call's scratch of before counted as free) hold them */
   uint64_t wanted = reduce->scratch_bytes;

   if (!wanted)
   {
      size_t freeBytes = 0, totalBytes = 0;

      HIP_TRY(ctx, hipMemGetInfo(&freeBytes, &totalBytes));
      wanted = totalBytes ? ((uint64_t)freeBytes + ctx->tapReduceScratchBytes) / 4 * 3 : ~0ull;
   }

   const uint32_t slabBuffers = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(wanted / bufferPitch, 1), nBuffers);

   uint64_t mostSegments = 0;

   for (uint64_t b0 = 0; b0 < nBuffers; b0 += slabBuffers)
   {
      uint64_t firstItem, items, segments;
      slab_plan((uint32_t)b0, (uint32_t)std::min<uint64_t>(b0 + slabBuffers, nBuffers), firstItem, items, segments);
      mostSegments = std::max(mostSegments, segments);
   }

   const size_t planesBytes = (size_t)(bufferPitch * slabBuffers);
   const size_t need = planesBytes + (size_t)mostSegments * K * sizeof(NfcTapPartial);

   if (need > ctx->tapReduceScratchBytes)
   {
      if (ctx->tapReduceScratch)
         (void)hipFree(ctx->tapReduceScratch);
      ctx->tapReduceScratch = nullptr;
      ctx->tapReduceScratchBytes = 0;
      if (hipMalloc(&ctx->tapReduceScratch, need) != hipSuccess)
         return fail(ctx, NFCGPU_ENOMEM, "tap reduce: scratch for the planes and the partials could not be allocated");
      ctx->tapReduceScratchBytes = need;
   }

   /* up: rows and state_in (host memory), the caller's ranges (host memory), the plan (order, prefix, table). down: the flag word; records and state_out
    * (host memory) */
   nfcgpu_ctx::StageSlot *up = nullptr, *down = nullptr;

   struct Release
   {
      nfcgpu_ctx *ctx;
      nfcgpu_ctx::StageSlot **up, **down;
      ~Release()
      {
         if (*up)
            stage_release(ctx, *up);
         if (*down)
            stage_release(ctx, *down);
      }
   } release {ctx, &up, &down};

   const size_t upPitch = (rowBytes + 255) & ~(size_t)255;
   const size_t rowsAt = 0, statesAt = rowsAt + (host ? upPitch * nBuffers : 0), rangesAt = statesAt + (host ? stateBytes : 0);
   const size_t orderAt = rangesAt + (host ? rangesBytes : 0), prefixAt = orderAt + round16((size_t)nRanges * 4u);
   const size_t tableAt = prefixAt + ((size_t)nRanges + 1) * 8u;
   const size_t upBytes = tableAt + table.size() * sizeof(NfcTapSegment) + 8;
   const size_t flagAt = 0, recordsAt = 16, statesOutAt = recordsAt + (host ? records * sizeof(NfcTapStat) : 0);
   const size_t downBytes = statesOutAt + (host ? stateBytes : 0);

   ctx->inflight = true;

   rc = stage_acquire(ctx, upBytes, &up);
   if (rc)
      return rc;
   rc = stage_acquire(ctx, downBytes, &down);
   if (rc)
      return rc;

   if (host)
   {
      for (uint32_t b = 0; b < nBuffers; b++)
         std::memcpy(up->h + rowsAt + (size_t)b * upPitch, (const uint8_t *)in + (size_t)b * inPitch, rowBytes);
      if (stateIn)
         std::memcpy(up->h + statesAt, stateIn, stateBytes);
      if (nRanges)
         std::memcpy(up->h + rangesAt, ranges, rangesBytes);
   }
   if (nRanges)
      std::memcpy(up->h + orderAt, order.data(), (size_t)nRanges * 4u);
   std::memcpy(up->h + prefixAt, prefix.data(), ((size_t)nRanges + 1) * 8u);
   if (!table.empty())
      std::memcpy(up->h + tableAt, table.data(), table.size() * sizeof(NfcTapSegment));

   HIP_TRY(ctx, hipMemcpyAsync(up->d, up->h, upBytes, hipMemcpyHostToDevice, ctx->stream));
   HIP_TRY(ctx, hipMemsetAsync(down->d + flagAt, 0, 16, ctx->stream));

   const uint8_t *dIn = host ? up->d + rowsAt : (const uint8_t *)in;
   const uint64_t dInPitch = host ? upPitch : inPitch;
   const NfcTapRecord *dStateIn = !stateIn ? nullptr : (host ? (const NfcTapRecord *)(up->d + statesAt) : (const NfcTapRecord *)stateIn);
   NfcTapRecord *dStateOut = !stateOut ? nullptr : (host ? (NfcTapRecord *)(down->d + statesOutAt) : (NfcTapRecord *)stateOut);

   NfcTapReduceArgs A;
   std::memset(&A, 0, sizeof(A));

   A.planes = (const float *)ctx->tapReduceScratch;
   A.partials = (NfcTapPartial *)((uint8_t *)ctx->tapReduceScratch + planesBytes);
   A.ranges = !ranges ? nullptr : (host ? (const NfcTapRange *)(up->d + rangesAt) : (const NfcTapRange *)ranges);
   A.order = (const uint32_t *)(up->d + orderAt);
   A.prefix = (const uint64_t *)(up->d + prefixAt);
   A.table = (const NfcTapSegment *)(up->d + tableAt);
   A.out = host ? (NfcTapStat *)(down->d + recordsAt) : (NfcTapStat *)out;
   A.flag = (uint32_t *)(down->d + flagAt);
   A.bufferPitch = bufferPitch;
   A.planePitch = planePitch;
   A.n = n;
   A.nBuffers = nBuffers;
   A.channels = K;
   A.binSamples = bin;
   A.bins = bins;
   A.segsPerBin = segsPerBin;

   nfcgpu_tap_report sum;
   std::memset(&sum, 0, sizeof(sum));

   for (uint64_t b0 = 0; b0 < nBuffers; b0 += slabBuffers)
   {
      const uint32_t b1 = (uint32_t)std::min<uint64_t>(b0 + slabBuffers, nBuffers);
      nfcgpu_tap_report one;
      uint64_t segments;

      /* stage 1: the slab's planes, by the tap itself (it returns when they are complete) */
      rc = nfcgpu_signal_tap(ctx, dIn + b0 * dInPitch, dInPitch, b1 - (uint32_t)b0, n, stride, format, tap, (const nfcgpu_tap_state *)(dStateIn ? dStateIn + b0 : nullptr),
                             (float *)ctx->tapReduceScratch, bufferPitch, planePitch, (nfcgpu_tap_state *)(dStateOut ? dStateOut + b0 : nullptr), &one, NFCGPU_LOC_DEVICE);
      if (rc)
         return rc;

      sum.chunks += one.chunks;
      sum.rounds += one.rounds;
      sum.rewalked_chunks += one.rewalked_chunks;

      /* stage 2: the ranges of the slab */
      A.b0 = (uint32_t)b0;
      A.b1 = b1;
      slab_plan(A.b0, A.b1, A.firstItem, A.items, segments);
      A.units = segments * K;
      A.prefix0 = ranges ? prefix[(size_t)A.firstItem] : 0;

      if (A.units)
      {
         const uint64_t blocks = (A.units + NfcTapReduceShape::kWaves - 1) / NfcTapReduceShape::kWaves;
         hipLaunchKernelGGL(nfc_tap_reduce_kernel, dim3((uint32_t)std::min(blocks, kTapReduceBlocks)), dim3(64 * NfcTapReduceShape::kWaves), 0, ctx->stream, A);
         HIP_TRY(ctx, hipGetLastError());
      }
      if (A.items)
      {
         const uint64_t blocks = (A.items * K + 255) / 256;
         hipLaunchKernelGGL(nfc_tap_reduce_finish_kernel, dim3((uint32_t)std::min<uint64_t>(blocks, 65536)), dim3(256), 0, ctx->stream, A);
         HIP_TRY(ctx, hipGetLastError());
      }
   }

   HIP_TRY(ctx, hipMemcpyAsync(down->h, down->d, downBytes, hipMemcpyDeviceToHost, ctx->stream));
   HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));

   if (host)
   {
      if (records)
         std::memcpy(out, down->h + recordsAt, records * sizeof(NfcTapStat));
      if (stateOut)
         std::memcpy(stateOut, down->h + statesOutAt, stateBytes);
   }

   if (report)
      *report = sum;

   if (*(const uint32_t *)(down->h + flagAt))
      return fail(ctx, NFCGPU_EINVAL, "tap reduce: a range in device memory is not inside the buffers or its reserved field is not zero; its records are empty");

   return NFCGPU_OK;
}

/* ---- nfcgpu_apcm_encode: the resampler's control points as the APCM entries of a trace file (nfc_apcm.hpp) ---- */

static_assert(sizeof(nfcgpu_apcm_info) == sizeof(NfcApcmInfo) && sizeof(NfcApcmInfo) == 16, "an APCM result record is 16 bytes");
static_assert(sizeof(nfcgpu_apcm_params) == 56 && sizeof(NfcApcmPair) == 8 && sizeof(NfcApcmPart) == 24 && sizeof(NfcApcmBase) == 16, "APCM structures");

constexpr uint64_t kApcmBlocks = 16384;   /* of four waves: the rest of the units by stride */

uint64_t nfcgpu_apcm_bound(uint64_t totalPairs)
{
   return NFC_APCM_HEADER_BYTES + 3u * totalPairs;
}

int nfcgpu_apcm_encode(nfcgpu_ctx *ctx, const float *pairs, uint64_t pairsPitch, const uint32_t *counts, uint32_t nBuffers, uint32_t capacityPairs,
                       const nfcgpu_apcm_params *params, void *out, uint64_t outPitch, uint64_t capacityBytes, nfcgpu_apcm_info *info, uint32_t location)
{
   SETTLE_FIRST(ctx);

   if (!ctx)
      return NFCGPU_EINVAL;
   if (!params)
      return fail(ctx, NFCGPU_EINVAL, "apcm: params is NULL");
   if (params->reserved0 | params->reserved[0] | params->reserved[1] | params->reserved[2] | params->reserved[3])
      return fail(ctx, NFCGPU_EINVAL, "apcm: reserved fields of params are not zero");
   if (location != NFCGPU_LOC_HOST && location != NFCGPU_LOC_DEVICE)
      return fail(ctx, NFCGPU_EINVAL, "apcm: unknown location");
   if (params->sample_rate == 0)
      return fail(ctx, NFCGPU_EINVAL, "apcm: sample rate 0");

   const uint32_t G = params->buffers_per_entry;

   if (G == 0 || nBuffers % G != 0)
      return fail(ctx, NFCGPU_EINVAL, "apcm: buffers_per_entry is 0 or does not divide n_buffers");
   if ((uint64_t)params->first_position + (uint64_t)G * params->buffer_samples > 0xFFFFFFFFull)
      return fail(ctx, NFCGPU_EINVAL, "apcm: the position of a buffer's end is not below 2^32");

   const uint32_t nEntries = nBuffers / G;

   if ((uint64_t)params->first_stream_id + nEntries > 0x100000000ull)
      return fail(ctx, NFCGPU_EINVAL, "apcm: a stream id is not below 2^32");

   /* the range in samples: the reference's product and cast (TraceStorageTask.cpp:907-908); 0, 0 is everything */
   const double start = (double)params->sample_rate * params->range_start, stop = (double)params->sample_rate * params->range_end;

   if (!(params->range_start >= 0.0) || !(params->range_end >= params->range_start) || !(stop < 4294967296.0))
      return fail(ctx, NFCGPU_EINVAL, "apcm: range_start and range_end are not 0 <= start <= end with sample_rate * end below 2^32");

   const bool everything = params->range_start == 0.0 && params->range_end == 0.0;

   if (((uintptr_t)pairs & 7) || (pairsPitch & 7) || pairsPitch < (uint64_t)capacityPairs * 8)
      return fail(ctx, NFCGPU_EINVAL, "apcm: pairs or pairs_pitch_bytes is not 8-byte aligned, or the pitch is smaller than capacity_pairs pairs");
   if (((uintptr_t)counts & 3) || ((uintptr_t)info & 3))
      return fail(ctx, NFCGPU_EINVAL, "apcm: counts or info is not 4-byte aligned");
   if (((uintptr_t)out & 3) || (outPitch & 3))
      return fail(ctx, NFCGPU_EINVAL, "apcm: out or out_pitch_bytes is not a multiple of 4");
   if (capacityBytes < NFC_APCM_HEADER_BYTES || outPitch < capacityBytes)
      return fail(ctx, NFCGPU_EINVAL, "apcm: capacity_bytes is below the 32 bytes of a header or above out_pitch_bytes");
   if ((uint64_t)G * capacityPairs > (0xFFFFFFFFull - NFC_APCM_HEADER_BYTES) / 3)
      return fail(ctx, NFCGPU_EINVAL, "apcm: the pairs of an entry (buffers_per_entry * capacity_pairs) need 4 GiB or more");

   if (nBuffers == 0)
      return NFCGPU_OK;

   if (!pairs || !counts || !out || !info)
      return fail(ctx, NFCGPU_EINVAL, "apcm: pairs, counts, out or info is NULL");

   const bool host = location == NFCGPU_LOC_HOST;

   if (host)
   {
      for (uint32_t b = 0; b < nBuffers; b++)
      {
         if (counts[b] > capacityPairs)
         {
            const std::string what = "apcm: the count of buffer " + std::to_string(b) + " is above capacity_pairs";
            return fail(ctx, NFCGPU_EINVAL, what.c_str());
         }
      }
   }

   HIP_TRY(ctx, hipSetDevice(ctx->device));

   NfcApcmArgs A;
   std::memset(&A, 0, sizeof(A));

   A.chunksPerBuffer = std::max<uint32_t>((uint32_t)(((uint64_t)capacityPairs + NfcApcmShape::kChunk - 1) / NfcApcmShape::kChunk), 1u);
   A.units = (uint64_t)nBuffers * A.chunksPerBuffer;
   A.unitsPerEntry = (uint64_t)G * A.chunksPerBuffer;
   A.nBuffers = nBuffers;
   A.nEntries = nEntries;
   A.capacityPairs = capacityPairs;
   A.buffersPerEntry = G;
   A.bufferSamples = params->buffer_samples;
   A.firstPosition = params->first_position;
   A.firstStreamId = params->first_stream_id;
   A.sampleRate = params->sample_rate;
   A.sampleStart = everything ? 0u : (uint32_t)start;
   A.sampleEnd = everything ? 0xFFFFFFFFu : (uint32_t)stop;
   A.maxRecords = (uint32_t)std::min<uint64_t>((capacityBytes - NFC_APCM_HEADER_BYTES) / 3, 0xFFFFFFFFull);

   /* scratch the context keeps: the flag word, the parts, the bases */
   const size_t partsAt = 16, basesAt = partsAt + (size_t)A.units * sizeof(NfcApcmPart), need = basesAt + (size_t)A.units * sizeof(NfcApcmBase);

   if (need > ctx->apcmScratchBytes)
   {
      if (ctx->apcmScratch)
         (void)hipFree(ctx->apcmScratch);
      ctx->apcmScratch = nullptr;
      ctx->apcmScratchBytes = 0;
      if (hipMalloc(&ctx->apcmScratch, need) != hipSuccess)
         return fail(ctx, NFCGPU_ENOMEM, "apcm: scratch for the units could not be allocated");
      ctx->apcmScratchBytes = need;
   }

   A.flag = (uint32_t *)ctx->apcmScratch;
   A.parts = (NfcApcmPart *)((uint8_t *)ctx->apcmScratch + partsAt);
   A.bases = (NfcApcmBase *)((uint8_t *)ctx->apcmScratch + basesAt);

   /* host memory: one temporary device block - the rows packed to capacity_pairs, the counts, the entries, the results (this
    * entry point is not on the streaming path) */
   const size_t rowBytes = (size_t)capacityPairs * 8, entryPitch = (size_t)((capacityBytes + 3) & ~(uint64_t)3);
   const size_t countsAt = rowBytes * nBuffers, entriesAt = (countsAt + (size_t)nBuffers * 4 + 15) & ~(size_t)15;
   const size_t infoAt = entriesAt + entryPitch * nEntries, blockBytes = infoAt + (size_t)nEntries * sizeof(NfcApcmInfo);
   uint8_t *block = nullptr;

   struct Release
   {
      uint8_t **block;
      ~Release()
      {
         if (*block)
            (void)hipFree(*block);
      }
   } release {&block};

   ctx->inflight = true;

   if (host)
   {
      if (hipMalloc((void **)&block, blockBytes) != hipSuccess)
         return fail(ctx, NFCGPU_ENOMEM, "apcm: device memory for host rows could not be allocated");

      std::vector<uint8_t> up(entriesAt, 0);

      for (uint32_t b = 0; b < nBuffers; b++)
         std::memcpy(up.data() + rowBytes * b, (const uint8_t *)pairs + (size_t)pairsPitch * b, (size_t)counts[b] * 8);
      std::memcpy(up.data() + countsAt, counts, (size_t)nBuffers * 4);

      HIP_TRY(ctx, hipMemcpy(block, up.data(), entriesAt, hipMemcpyHostToDevice));

      A.pairs = block;
      A.pairsPitch = rowBytes;
      A.counts = (const uint32_t *)(block + countsAt);
      A.out = block + entriesAt;
      A.outPitch = entryPitch;
      A.info = (NfcApcmInfo *)(block + infoAt);
   }
   else
   {
      A.pairs = (const uint8_t *)pairs;
      A.pairsPitch = pairsPitch;
      A.counts = counts;
      A.out = (uint8_t *)out;
      A.outPitch = outPitch;
      A.info = (NfcApcmInfo *)info;
   }

   HIP_TRY(ctx, hipMemsetAsync(A.flag, 0, 16, ctx->stream));

   const uint32_t unitBlocks = (uint32_t)std::min<uint64_t>((A.units + NfcApcmShape::kWaves - 1) / NfcApcmShape::kWaves, kApcmBlocks);

   hipLaunchKernelGGL(nfc_apcm_count_kernel, dim3(unitBlocks), dim3(64 * NfcApcmShape::kWaves), 0, ctx->stream, A);
   HIP_TRY(ctx, hipGetLastError());
   hipLaunchKernelGGL(nfc_apcm_scan_kernel, dim3(std::min<uint32_t>(nEntries, 65536u)), dim3(64), 0, ctx->stream, A);
   HIP_TRY(ctx, hipGetLastError());
   hipLaunchKernelGGL(nfc_apcm_encode_kernel, dim3(unitBlocks), dim3(64 * NfcApcmShape::kWaves), 0, ctx->stream, A);
   HIP_TRY(ctx, hipGetLastError());

   /* the results as the host sees them: what the call returns depends on them */
   std::vector<NfcApcmInfo> results(nEntries);
   uint32_t flag = 0;

   HIP_TRY(ctx, hipMemcpyAsync(results.data(), A.info, (size_t)nEntries * sizeof(NfcApcmInfo), hipMemcpyDeviceToHost, ctx->stream));
   HIP_TRY(ctx, hipMemcpyAsync(&flag, A.flag, 4, hipMemcpyDeviceToHost, ctx->stream));
   HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));

   bool overflow = false;

   for (uint32_t e = 0; e < nEntries; e++)
      overflow = overflow || results[e].records > A.maxRecords;

   if (host)
   {
      /* an entry's bytes and no others: what lies behind them in the caller's pitch is left alone */
      std::vector<uint8_t> down(entryPitch * nEntries);

      HIP_TRY(ctx, hipMemcpy(down.data(), A.out, down.size(), hipMemcpyDeviceToHost));

      for (uint32_t e = 0; e < nEntries; e++)
         std::memcpy((uint8_t *)out + (size_t)outPitch * e, down.data() + entryPitch * e,
                     NFC_APCM_HEADER_BYTES + 3u * (size_t)std::min(results[e].records, A.maxRecords));
      std::memcpy(info, results.data(), (size_t)nEntries * sizeof(NfcApcmInfo));
   }

   if (flag)
      return fail(ctx, NFCGPU_EINVAL, "apcm: a count in device memory is above capacity_pairs; capacity_pairs pairs of that buffer were taken");
   if (overflow)
      return fail(ctx, NFCGPU_EOVERFLOW, "apcm: an entry needs more than capacity_bytes: its info says how many");

   return NFCGPU_OK;
}

int nfcgpu_stream_tap_state(nfcgpu_ctx *ctx, uint32_t id, nfcgpu_tap_state *state)
{
   SETTLE_FIRST(ctx);

   if (!ctx || !state)
      return NFCGPU_EINVAL;
   if (id >= ctx->maxStreams || !ctx->streams[id].open)
      return fail(ctx, NFCGPU_ESTREAM, "unknown stream");

   int rc = nfcgpu_sync(ctx);
   if (rc && rc != NFCGPU_EOVERFLOW)
      return rc;

   const StreamInfo &si = ctx->streams[id];

   nfcgpu_tap_state_init(state);

   /* a stream never fed starts from nothing; a pending initialize() restarts the clock and carries the front end on (nfc_state_init) */
   if (si.initialized)
   {
      NfcTapState s;
      HIP_TRY(ctx, hipMemcpy(&s, ctx->dStates + id, sizeof(s), hipMemcpyDeviceToHost));
      std::memcpy(state, &s, sizeof(s));
      if (si.needInit)
         state->clock = 0xFFFFFFFFu;
   }

   return rc;
}

int nfcgpu_submit_uniform(nfcgpu_ctx *ctx, uint32_t first, uint32_t count, const void *base, uint64_t pitch, uint32_t n,
                          uint32_t stride, uint32_t location, uint32_t sampleRate)
{
   return nfcgpu_submit_uniform_fmt(ctx, first, count, base, pitch, n, stride, location, sampleRate, NFCGPU_FMT_F32);
}

int nfcgpu_submit_uniform_fmt(nfcgpu_ctx *ctx, uint32_t first, uint32_t count, const void *base, uint64_t pitch, uint32_t n,
                              uint32_t components, uint32_t location, uint32_t sampleRate, uint32_t format)
{
   if (!ctx || !base || (components != 1 && components != 2) || count == 0 || (format != NFCGPU_FMT_F32 && format != NFCGPU_FMT_I16) ||
       (location != NFCGPU_LOC_HOST && location != NFCGPU_LOC_DEVICE))
      return NFCGPU_EINVAL;

   /* the sample layout of the rows (nfc_sample.hpp): the components per sample themselves for floats */
   const uint32_t stride = components | (format == NFCGPU_FMT_I16 ? NFC_SAMPLE_I16 : 0u);
   const uint32_t sampleBytes = nfc_sample_bytes(stride);

   if (count > 1 && pitch < (uint64_t)n * sampleBytes)
      return NFCGPU_EINVAL;
   if ((uint64_t)first + count > ctx->maxStreams)
      return fail(ctx, NFCGPU_ESTREAM, "stream range out of bounds");

   /* rows are read as float2 (IQ) or float, as pairs of int16 or int16: base and pitch have to be aligned to a sample */
   if (((uintptr_t)base % sampleBytes) != 0 || (count > 1 && (pitch % sampleBytes) != 0))
      return fail(ctx, NFCGPU_EINVAL, format == NFCGPU_FMT_I16 ? "base and pitch must be multiples of the sample size (2 bytes int16 magnitude, 4 bytes int16 IQ)"
                                                                : "base and pitch must be multiples of the sample size (4 bytes magnitude, 8 bytes IQ)");

#ifdef NFCGPU_EMULATED_TEST_BUILD
   /* (test scaffolding: see widen_i16) */
   if (format == NFCGPU_FMT_I16)
   {
      const size_t row = (size_t)n * components;
      ctx->widened.emplace_back(row * count + 2);
      float *wide = ctx->widened.back().data();
      for (uint32_t r = 0; r < count; r++)
         for (size_t i = 0; i < row; i++)
            wide[(size_t)r * row + i] = nfc_i16_to_float(((const int16_t *)((const uint8_t *)base + (size_t)r * pitch))[i]);
      return nfcgpu_submit_uniform_fmt(ctx, first, count, wide, row * 4, n, components, location, sampleRate, NFCGPU_FMT_F32);
   }
#endif

   HIP_TRY(ctx, hipSetDevice(ctx->device));

   /* A pending tail (run_windowed) is completed first - unless this submission may run its front under it: the very streams of
    * the pending one, none of them with an initialisation pending or a changed sample rate. (What else stands in the way -
    * another configuration, a clock near the wrap - is found further down, and the tail completed there.) */
   if (ctx->tail)
   {
      bool candidate = ctx->pipeline && n != 0 && first == ctx->tail->items.front().slot && count == ctx->tail->items.size();

      for (uint32_t i = first; candidate && i < first + count; i++)
      {
         const StreamInfo &si = ctx->streams[i];
         candidate = si.open && si.initialized && !si.needInit && si.derivedRate != 0 && si.params.sample_rate == sampleRate;
      }

      if (!candidate)
      {
         int rc = settle_tail(ctx);
         if (rc)
            return rc;
      }
   }

   /* an empty buffer still stores a new sample rate and re-initialises the stream, like nfcgpu_submit (NfcDecoder.cpp:383-388) */
   for (uint32_t i = first; i < first + count; i++)
   {
      if (!ctx->streams[i].open)
         return fail(ctx, NFCGPU_ESTREAM, "closed stream inside uniform range");

      int rc = adopt_sample_rate(ctx, ctx->streams[i], sampleRate);
      if (rc)
         return rc;
   }

   if (n == 0)
      return NFCGPU_OK;

   const uint8_t *devBase = (const uint8_t *)base;
   uint64_t devPitch = pitch;
   nfcgpu_ctx::StageSlot *slot = nullptr;

   ctx->inflight = true;

   /* host rows go through a staging slot; its event is recorded behind whatever this call enqueues, on every exit */
   struct Release
   {
      nfcgpu_ctx *ctx;
      nfcgpu_ctx::StageSlot *slot;
      ~Release() { if (slot) stage_release(ctx, slot); }
   } release {ctx, nullptr};

   if (location == NFCGPU_LOC_HOST)
   {
      const size_t row = (size_t)n * sampleBytes;
      devPitch = (row + 255) & ~(size_t)255;

      int rc = stage_acquire(ctx, devPitch * count, &slot);
      if (rc)
         return rc;

      for (uint32_t r = 0; r < count; r++)
         std::memcpy(slot->h + (size_t)r * devPitch, (const uint8_t *)base + (size_t)r * pitch, row);

      release.slot = slot;

      if (ctx->tail)
      {
         /* (the main stream is the pending tail's: the rows go up on the stream the front will run on, and whatever takes them
          * from the main stream after all waits for that) */
         HIP_TRY(ctx, hipMemcpyAsync(slot->d, slot->h, devPitch * count, hipMemcpyHostToDevice, ctx->front));
         HIP_TRY(ctx, hipEventRecord(ctx->frontEvent, ctx->front));
         HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->frontEvent, 0));
      }
      else
         HIP_TRY(ctx, hipMemcpyAsync(slot->d, slot->h, devPitch * count, hipMemcpyHostToDevice, ctx->stream));
      devBase = slot->d;
   }

   int rc = initialize_pending(ctx, first, count, false);
   if (rc)
      return rc;

   /* (a submission of this kind may leave its tail pending: run_windowed) */
   struct Deferring
   {
      nfcgpu_ctx *ctx;
      ~Deferring() { ctx->deferOK = false; }
   } deferring {ctx};
   ctx->deferOK = true;

   rc = run_rows(ctx, first, count, devBase, devPitch, n, stride);
   if (rc)
      return rc;

   /* the staging slot stays held until the pending tail is done: its kernels read the rows */
   if (ctx->tail && release.slot)
   {
      ctx->tail->slot = release.slot;
      release.slot = nullptr;
   }

   /* host buffers are never retained past the call: they were copied into the staging slot */
   return NFCGPU_OK;
}

int nfcgpu_sync(nfcgpu_ctx *ctx)
{
   SETTLE_FIRST(ctx);

   if (!ctx)
      return NFCGPU_EINVAL;


   /* nothing enqueued since the last synchronisation and nothing to collect: no device call at all */
   if (!ctx->inflight && !ctx->dirty && ctx->timed.empty() && ctx->timedScan.empty() && ctx->timedWindow.empty() && ctx->timedWave.empty() && ctx->timedPlanes.empty())
      return NFCGPU_OK;

   HIP_TRY(ctx, hipSetDevice(ctx->device));
   HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
   ctx->inflight = false;
#ifdef NFCGPU_EMULATED_TEST_BUILD
   ctx->widened.clear(); /* (test scaffolding: widen_i16) */
#endif

   if (!ctx->timedWave.empty() || !ctx->timedPlanes.empty())
      (void)hipStreamSynchronize(ctx->side); /* (carry lanes run beside the windows) */

   collect_timings(ctx);

   if (!ctx->dirty || ctx->hold)
      return NFCGPU_OK;

   uint32_t ctl[2] = {0, 0};
   HIP_TRY(ctx, hipMemcpy(ctl, ctx->dSinkCtl, sizeof(ctl), hipMemcpyDeviceToHost));

   const uint64_t used = ctl[0] < ctx->sinkWords ? ctl[0] : ctx->sinkWords;

   if (used)
   {
      ctx->hSink.resize(used);
      HIP_TRY(ctx, hipMemcpy(ctx->hSink.data(), ctx->dSink, used * 4, hipMemcpyDeviceToHost));
      drain_sink(ctx, ctl[0]);
   }

   ctx->stats.dropped_frames += ctl[1];

   HIP_TRY(ctx, hipMemsetAsync(ctx->dSinkCtl, 0, 16, ctx->stream));
   HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));

   ctx->dirty = false;

   if (ctl[1])
      return fail(ctx, NFCGPU_EOVERFLOW, "frame sink overflow: frames were dropped (raise frame_sink_bytes or sync more often)");

   return NFCGPU_OK;
}

int nfcgpu_flush(nfcgpu_ctx *ctx, uint32_t id)
{
   if (!ctx)
      return NFCGPU_EINVAL;
   if (id >= ctx->maxStreams || !ctx->streams[id].open)
      return fail(ctx, NFCGPU_ESTREAM, "unknown stream");

   int rc = nfcgpu_sync(ctx);
   if (rc && rc != NFCGPU_EOVERFLOW)
      return rc;

   StreamInfo &si = ctx->streams[id];

   uint32_t clock = 0xFFFFFFFFu, carrierOn = 0;

   if (si.initialized)
   {
      NfcStreamState s;
      HIP_TRY(ctx, hipMemcpy(&s, ctx->dStates + id, sizeof(s), hipMemcpyDeviceToHost));
      clock = si.needInit ? 0xFFFFFFFFu : s.clock; /* a pending initialize() has already reset the clock, not the carrier state */
      carrierOn = s.carrierOn;
   }

   nfcgpu_frame f;
   std::memset(&f, 0, sizeof(f));
   f.stream_id = id;
   f.tech_type = NFC_TECH_ANY;
   f.frame_type = carrierOn ? NFC_FRAME_CARRIER_ON : NFC_FRAME_CARRIER_OFF;
   f.frame_phase = NFC_PHASE_CARRIER;
   f.sample_start = clock;
   f.sample_end = clock;
   f.sample_rate = si.params.sample_rate;

   si.queue.push_back(f);
   return rc;
}

int nfcgpu_poll(nfcgpu_ctx *ctx, uint32_t id, nfcgpu_frame *out, uint32_t capacity, uint32_t *count)
{
   if (!ctx || !count || (capacity && !out))
      return NFCGPU_EINVAL;
   if (id >= ctx->maxStreams || !ctx->streams[id].open)
      return fail(ctx, NFCGPU_ESTREAM, "unknown stream");

   int rc = nfcgpu_sync(ctx);
   if (rc && rc != NFCGPU_EOVERFLOW)
      return rc;

   StreamInfo &si = ctx->streams[id];
   uint32_t n = 0;

   while (n < capacity && !si.queue.empty())
   {
      out[n++] = si.queue.front();
      si.queue.pop_front();
   }

   *count = n;
   return rc;
}

/* the frames the device has decoded for a stream, as the trace file the reference application opens
 * (TraceStorageTask.cpp:211-240 the range of "write file", 461-520 the entries). The frames stay in the stream's queue. */
int nfcgpu_trace_write(nfcgpu_ctx *ctx, uint32_t id, const char *path, double rangeStart, double rangeEnd, uint32_t *written)
{
   if (!ctx || !path)
      return NFCGPU_EINVAL;
   if (id >= ctx->maxStreams || !ctx->streams[id].open)
      return fail(ctx, NFCGPU_ESTREAM, "unknown stream");

   /* (a held sink is not drained by nfcgpu_sync: the stream's queue would be empty and the file with it) */
   if (ctx->hold)
      return fail(ctx, NFCGPU_EINVAL, "nfcgpu_trace_write while the sink is held (nfcgpu_sink_hold): the frames are in the caller's sink, not in the stream's queue");

   int rc = nfcgpu_sync(ctx);
   if (rc && rc != NFCGPU_EOVERFLOW)
      return rc;

   const StreamInfo &si = ctx->streams[id];
   std::vector<nfcgpu_frame> frames(si.queue.begin(), si.queue.end());

   const int wrote = nfcgpu_trace_write_frames(path, frames.data(), (uint32_t)frames.size(), si.params.stream_time, rangeStart, rangeEnd, written);
   if (wrote)
      return fail(ctx, wrote, "the trace file could not be written");

   return rc;
}

int nfcgpu_pending(nfcgpu_ctx *ctx, uint32_t id, uint32_t *count)
{
   if (!ctx || !count)
      return NFCGPU_EINVAL;
   if (id >= ctx->maxStreams || !ctx->streams[id].open)
      return fail(ctx, NFCGPU_ESTREAM, "unknown stream");

   int rc = nfcgpu_sync(ctx);
   *count = (uint32_t)ctx->streams[id].queue.size();
   return rc;
}

int nfcgpu_sink_device_view(nfcgpu_ctx *ctx, const void **words, const void **cursor, uint64_t *capacity)
{
   SETTLE_FIRST(ctx);

   if (!ctx)
      return NFCGPU_EINVAL;

   if (words)
      *words = ctx->dSink;
   if (cursor)
      *cursor = ctx->dSinkCtl;
   if (capacity)
      *capacity = ctx->sinkWords;
   return NFCGPU_OK;
}

int nfcgpu_sink_attach(nfcgpu_ctx *ctx, void *words, uint64_t capacityWords, void *ctl)
{
   SETTLE_FIRST(ctx);

   if (!ctx || (words && (!ctl || capacityWords < 4ull * NFC_FRAME_MAX_WORDS || capacityWords > 0xFFFFFFF0ull)))
      return NFCGPU_EINVAL;


   const bool wasHeld = ctx->hold;
   ctx->hold = false;
   int rc = nfcgpu_sync(ctx); /* drain what the current sink holds */
   ctx->hold = wasHeld;

   if (rc && rc != NFCGPU_EOVERFLOW)
      return rc;

   if (words)
   {
      ctx->dSink = (uint32_t *)words;
      ctx->dSinkCtl = (uint32_t *)ctl;
      ctx->sinkWords = capacityWords;
   }
   else
   {
      ctx->dSink = ctx->ownSink;
      ctx->dSinkCtl = ctx->ownSinkCtl;
      ctx->sinkWords = ctx->ownSinkWords;
   }

   return nfcgpu_sink_rewind(ctx);
}

int nfcgpu_sink_hold(nfcgpu_ctx *ctx, int hold)
{
   SETTLE_FIRST(ctx);

   if (!ctx)
      return NFCGPU_EINVAL;

   ctx->hold = hold != 0;
   return NFCGPU_OK;
}

int nfcgpu_sink_rewind(nfcgpu_ctx *ctx)
{
   SETTLE_FIRST(ctx);

   if (!ctx)
      return NFCGPU_EINVAL;

   HIP_TRY(ctx, hipSetDevice(ctx->device));
   HIP_TRY(ctx, hipMemsetAsync(ctx->dSinkCtl, 0, 16, ctx->stream));
   HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
   ctx->dirty = false;
   return NFCGPU_OK;
}


int nfcgpu_comm_unique_id(void *id128)
{
   if (!id128)
      return NFCGPU_EINVAL;
   Rccl *r = rccl();
   if (!r)
      return NFCGPU_ENODEV;
   return r->getUniqueId(id128) == 0 ? NFCGPU_OK : NFCGPU_EHIP;
}

int nfcgpu_comm_init(nfcgpu_ctx *ctx, const void *id128, int rank, int nRanks)
{
   SETTLE_FIRST(ctx);

   if (!ctx || !id128 || nRanks < 1 || rank < 0 || rank >= nRanks)
      return NFCGPU_EINVAL;

   Rccl *r = rccl();
   if (!r)
      return fail(ctx, NFCGPU_ENODEV, "librccl.so not found");

   HIP_TRY(ctx, hipSetDevice(ctx->device));

   if (ctx->comm)
      nfcgpu_comm_destroy(ctx);

   IdByValue id;
   std::memcpy(id.internal, id128, NFCGPU_UNIQUE_ID_BYTES);

   const int rc = r->commInitRank(&ctx->comm, nRanks, id, rank);
   if (rc != 0)
   {
      ctx->comm = nullptr;
      return fail(ctx, NFCGPU_EHIP, r->getErrorString ? r->getErrorString(rc) : "ncclCommInitRank failed");
   }

   ctx->commRank = rank;
   ctx->commRanks = nRanks;

   if (hipMalloc((void **)&ctx->dCounts, 8 * (size_t)(nRanks + 1)) != hipSuccess)
      return fail(ctx, NFCGPU_ENOMEM, "hipMalloc(gather counts)");

   return NFCGPU_OK;
}

int nfcgpu_comm_destroy(nfcgpu_ctx *ctx)
{
   SETTLE_FIRST(ctx);

   if (!ctx)
      return NFCGPU_EINVAL;

   /* (librccl.so is only looked up for a context that has a communicator: a plain shutdown - possibly from an atexit
    * handler of the host - must not load a library) */
   Rccl *r = ctx->comm ? rccl() : nullptr;

   if (ctx->comm && r)
   {
      (void)hipSetDevice(ctx->device);
      (void)hipStreamSynchronize(ctx->stream);
      (void)r->commDestroy(ctx->comm);
   }

   ctx->comm = nullptr;
   ctx->commRanks = 0;

   if (ctx->dCounts)
      (void)hipFree(ctx->dCounts);
   ctx->dCounts = nullptr;

   return NFCGPU_OK;
}

/* both forms of the gather: `packed` - rank r's records start at the sum of the counts before it; otherwise at r * stride,
 * stride = the largest count (the layout of rounds 1-2, kept under the old symbol) */
static int gather_frames(nfcgpu_ctx *ctx, void *gathered, uint64_t capacityWords, uint32_t *countsHost, uint64_t *strideWords, bool packed)
{
   SETTLE_FIRST(ctx);

   if (!ctx || !gathered || !countsHost || (!packed && !strideWords))
      return NFCGPU_EINVAL;

   if (!ctx->comm)
      return fail(ctx, NFCGPU_EINVAL, "nfcgpu_comm_init first");
   if (!ctx->hold)
      return fail(ctx, NFCGPU_EINVAL, "nfcgpu_sink_hold first: a sink that nfcgpu_sync drains has nothing left to gather");

   Rccl *r = rccl();
   if (!r)
      return fail(ctx, NFCGPU_ENODEV, "librccl.so not found");

   HIP_TRY(ctx, hipSetDevice(ctx->device));
   HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));

   /* this rank's records: what the sink holds, clamped like drain_sink does (a record is only ever written below
    * sinkWords - NFC_FRAME_MAX_WORDS) */
   uint32_t ctl[2] = {0, 0};
   HIP_TRY(ctx, hipMemcpy(ctl, ctx->dSinkCtl, sizeof(ctl), hipMemcpyDeviceToHost));

   uint64_t used = ctl[0];
   const uint64_t limit = ctx->sinkWords >= NFC_FRAME_MAX_WORDS ? ctx->sinkWords - NFC_FRAME_MAX_WORDS + 1 : 0;
   if (ctl[1] && used > limit)
      used = limit; /* dropped frames: everything that starts below the limit is whole (nfc_emit) */
   if (used > ctx->sinkWords)
      used = ctx->sinkWords;

   const int n = ctx->commRanks;

   /* Every rank learns every rank's word count AND what every rank's receive buffer holds: the decision to go on is
    * then the same on all of them (a rank that returned between the two collectives would leave the others waiting). */
   const uint32_t mine[2] = {(uint32_t)used, (uint32_t)(capacityWords > 0xFFFFFFFFull ? 0xFFFFFFFFull : capacityWords)};

   HIP_TRY(ctx, hipMemcpyAsync(ctx->dCounts + 2 * n, mine, 8, hipMemcpyHostToDevice, ctx->stream));
   int rc = r->allGather(ctx->dCounts + 2 * n, ctx->dCounts, 2, /* ncclUint32 */ 3, ctx->comm, ctx->stream);
   if (rc != 0)
      return fail(ctx, NFCGPU_EHIP, r->getErrorString ? r->getErrorString(rc) : "ncclAllGather(counts) failed");

   std::vector<uint32_t> pairs(2 * (size_t)n);
   HIP_TRY(ctx, hipMemcpyAsync(pairs.data(), ctx->dCounts, 8 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
   HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));

   uint64_t total = 0, smallest = ~0ull, largest = 0;
   for (int i = 0; i < n; i++)
   {
      countsHost[i] = pairs[2 * i];
      total += pairs[2 * i];
      largest = pairs[2 * i] > largest ? pairs[2 * i] : largest;
      smallest = pairs[2 * i + 1] < smallest ? pairs[2 * i + 1] : smallest;
   }

   const uint64_t stride = packed ? 0 : largest;
   const uint64_t needed = packed ? total : largest * (uint64_t)n;

   if (strideWords)
      *strideWords = stride;

   if (needed > smallest)
      return fail(ctx, NFCGPU_ENOMEM, "a rank's gather buffer is too small for all ranks' records (the same verdict on every rank)");

   /* records, exact sizes: one broadcast per rank into its place, all in one group */
   rc = r->groupStart();
   uint64_t at = 0;
   for (int i = 0; i < n && rc == 0; i++)
   {
      if (countsHost[i])
         rc = r->broadcast(ctx->dSink, (uint32_t *)gathered + (packed ? at : (uint64_t)i * stride), countsHost[i], /* ncclUint32 */ 3, i, ctx->comm, ctx->stream);
      at += countsHost[i];
   }
   const int rcEnd = r->groupEnd();
   if (rc == 0)
      rc = rcEnd;
   if (rc != 0)
      return fail(ctx, NFCGPU_EHIP, r->getErrorString ? r->getErrorString(rc) : "ncclBroadcast(records) failed");

   HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));

   return ctl[1] ? NFCGPU_EOVERFLOW : NFCGPU_OK;
}

int nfcgpu_gather_frames_packed(nfcgpu_ctx *ctx, void *gathered, uint64_t capacityWords, uint32_t *countsHost)
{
   return gather_frames(ctx, gathered, capacityWords, countsHost, nullptr, true);
}

int nfcgpu_gather_frames(nfcgpu_ctx *ctx, void *gathered, uint64_t capacityWords, uint32_t *countsHost, uint64_t *strideWords)
{
   return gather_frames(ctx, gathered, capacityWords, countsHost, strideWords, false);
}

int nfcgpu_read_bandwidth(nfcgpu_ctx *ctx, const void *ptr, uint64_t bytes, uint32_t repeats, double *gbps)
{
   SETTLE_FIRST(ctx);

   if (!ctx || !ptr || bytes < 16 || !gbps || ((uintptr_t)ptr & 15))
      return NFCGPU_EINVAL;


   HIP_TRY(ctx, hipSetDevice(ctx->device));

   float *out = nullptr;
   HIP_TRY(ctx, hipMalloc((void **)&out, 16));

   hipEvent_t a = take_event(ctx), b = take_event(ctx);
   double best = 0.0;

   for (uint32_t i = 0; i < (repeats ? repeats : 1); i++)
   {
      (void)hipEventRecord(a, ctx->stream);
      hipLaunchKernelGGL(nfc_read_kernel, dim3(256 * 16), dim3(256), 0, ctx->stream, (const float4 *)ptr, bytes / 16, out);
      (void)hipEventRecord(b, ctx->stream);
      (void)hipStreamSynchronize(ctx->stream);

      float ms = 0;
      if (hipEventElapsedTime(&ms, a, b) == hipSuccess && ms > 0)
      {
         const double g = (double)(bytes / 16 * 16) / (ms * 1e-3) / 1e9;
         best = g > best ? g : best;
      }
   }

   ctx->eventPool.push_back(a);
   ctx->eventPool.push_back(b);
   (void)hipFree(out);

   *gbps = best;
   return NFCGPU_OK;
}

namespace {

/* total length of the union of the wave decoder's launch intervals */
void close_wave_spans(nfcgpu_ctx *ctx)
{
   std::vector<std::pair<float, float>> &v = ctx->waveSpans;
   std::sort(v.begin(), v.end());

   double busy = ctx->waveBusyMs; /* (what fold_wave_spans has taken out of the list) */
   float lo = 0, hi = -1.0f;

   for (const auto &span: v)
   {
      if (hi < lo || span.first > hi)
      {
         if (hi >= lo)
            busy += hi - lo;
         lo = span.first;
         hi = span.second;
      }
      else if (span.second > hi)
         hi = span.second;
   }

   if (hi >= lo)
      busy += hi - lo;

   ctx->stats.wave_busy_ms = busy;
}

}

int nfcgpu_stats_get(nfcgpu_ctx *ctx, nfcgpu_stats *stats)
{
   SETTLE_FIRST(ctx);

   if (!ctx || !stats)
      return NFCGPU_EINVAL;

   std::memcpy(stats, &ctx->stats, NFCGPU_STATS_SIZE_V2); /* a caller built against the older header holds no more */
   return NFCGPU_OK;
}

int nfcgpu_stats_get_sized(nfcgpu_ctx *ctx, void *stats, uint32_t size)
{
   SETTLE_FIRST(ctx);

   if (!ctx || !stats)
      return NFCGPU_EINVAL;

   close_wave_spans(ctx);

   std::memcpy(stats, &ctx->stats, size < sizeof(nfcgpu_stats) ? size : sizeof(nfcgpu_stats));
   return NFCGPU_OK;
}

int nfcgpu_stats_reset(nfcgpu_ctx *ctx)
{
   SETTLE_FIRST(ctx);

   if (!ctx)
      return NFCGPU_EINVAL;

   ctx->stats = nfcgpu_stats();
   ctx->waveSpans.clear();
   ctx->waveBusyMs = 0.0;

   /* the time base of the launch intervals: an event on the context's stream, now (on the context's device: with several
    * contexts in a process - a rank per GPU - another one may be current) */
   HIP_TRY(ctx, hipSetDevice(ctx->device));
   if (!ctx->epoch)
      HIP_TRY(ctx, hipEventCreate(&ctx->epoch));
   HIP_TRY(ctx, hipEventRecord(ctx->epoch, ctx->stream));

   return NFCGPU_OK;
}

int nfcgpu_profile(nfcgpu_ctx *ctx, int enable)
{
   if (!ctx)
      return NFCGPU_EINVAL;

   ctx->profile = enable != 0;
   return NFCGPU_OK;
}

void *nfcgpu_hip_stream(nfcgpu_ctx *ctx)
{
   return ctx ? (void *)ctx->stream : nullptr;
}

const char *nfcgpu_strerror(int code)
{
   switch (code)
   {
      case NFCGPU_OK: return "ok";
      case NFCGPU_EINVAL: return "invalid argument";
      case NFCGPU_ENODEV: return "no usable HIP device (this library has no CPU fallback)";
      case NFCGPU_ENOMEM: return "out of memory";
      case NFCGPU_ESTREAM: return "unknown or closed stream";
      case NFCGPU_ERATE: return "sample rate not decodable";
      case NFCGPU_EOVERFLOW: return "frame sink overflow, frames dropped";
      case NFCGPU_EHIP: return "HIP runtime error";
      case NFCGPU_EFULL: return "no free stream slot";
      case NFCGPU_EIO: return "a file could not be opened or written";
      default: return "unknown error";
   }
}

const char *nfcgpu_last_error(nfcgpu_ctx *ctx)
{
   return ctx ? ctx->lastError.c_str() : "";
}

#ifdef NFCGPU_EMULATED_TEST_BUILD
/* TEST HOOKS, only in the emulated build of tests/hostsim (device memory is host memory there): place a stream's sample
 * clock (device record and host mirror) anywhere, e.g. next to the 32-bit wrap, and read it back. The reference offers no
 * way to preset its clock, so the product has none either. */
int nfcgpu_test_set_clock(nfcgpu_ctx *ctx, uint32_t id, uint32_t clock)
{
   SETTLE_FIRST(ctx);

   if (!ctx || id >= ctx->maxStreams || !ctx->streams[id].open || !ctx->streams[id].initialized)
      return NFCGPU_ESTREAM;
   ctx->dStates[id].clock = clock;
   ctx->streams[id].clock = clock;
   return NFCGPU_OK;
}

int nfcgpu_test_get_clock(nfcgpu_ctx *ctx, uint32_t id, uint32_t *device, uint32_t *mirror)
{
   SETTLE_FIRST(ctx);

   if (!ctx || id >= ctx->maxStreams || !device || !mirror)
      return NFCGPU_ESTREAM;
   *device = ctx->dStates[id].clock;
   *mirror = ctx->streams[id].clock;
   return NFCGPU_OK;
}
#endif

const char *nfcgpu_version(void)
{
#ifdef NFCGPU_EMULATED_TEST_BUILD
   return "nfcgpu 0.1 (test build of the host runtime on an emulated HIP: not a product library)";
#else
   return "nfcgpu 0.1 (gfx950)";
#endif
}

}

namespace {

/* rows first .. first + count - 1 of a uniform submission resident on the device: contiguous runs of one configuration ->
 * one launch each (normally exactly one) */
int run_rows(nfcgpu_ctx *ctx, uint32_t first, uint32_t count, const uint8_t *devBase, uint64_t devPitch, uint32_t n, uint32_t stride)
{
   int rc = NFCGPU_OK;
   uint32_t i = first;

   while (i < first + count)
   {
      const uint32_t c = ctx->streams[i].config;
      uint32_t j = i;

      while (j < first + count && ctx->streams[j].config == c)
         j++;

      {
         std::vector<WindowedItem> items(j - i);
         for (uint32_t k = i; k < j; k++)
            items[k - i] = WindowedItem {k, devBase + (uint64_t)(k - first) * devPitch, n};

         if (windowed_eligible(ctx, c, items))
         {
            rc = run_windowed(ctx, c, items, stride);
            if (rc)
               return rc;

            i = j;
            continue;
         }
      }

      if ((rc = settle_tail(ctx)))
         return rc;

      NfcLaunch L = base_launch(ctx);
      L.works = nullptr;
      L.uniformBase = devBase + (uint64_t)(i - first) * devPitch;
      L.uniformPitch = devPitch;
      L.uniformCount = n;
      L.uniformStride = stride;
      L.firstSlot = i;
      L.slotCount = j - i;

      bool exactPossible = false, exactOnly = true;
      for (uint32_t k = i; k < j; k++)
      {
         const bool exact = exact_zone(ctx->streams[k].clock, n);
         exactPossible = exactPossible || exact;
         exactOnly = exactOnly && exact;
      }

      rc = launch_demod(ctx, c, L, (uint64_t)n * (j - i), exactPossible, exactOnly);
      if (rc)
         return rc;

      for (uint32_t k = i; k < j; k++)
         commit_clock(ctx->streams[k], n);

      i = j;
   }

   return NFCGPU_OK;
}

}
