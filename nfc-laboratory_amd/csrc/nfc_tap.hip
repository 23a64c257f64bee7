/*
 * nfc_tap.hip - device kernels of nfcgpu_signal_tap: the front end's per-sample signals as planes of floats, cut in time and
 * exact. What a walker does and how its run is cut is nfc_tap.hpp; this file adds the grid, LDS and the barriers.
 *
 * nfc_tap_walk_kernel: a workgroup is one wave, 64 walkers, a lane each; groups of 64 walkers over the grid. Per tile of 16
 * samples: the wave fetches 64 runs of 16 samples (a load instruction takes four runs of 64 contiguous bytes of float input)
 * into a 64 x 17 tile of LDS, each lane walks its row through the decoder's front end (nfc_front_end_core, the configuration
 * in the kernel's arguments: scalar loads of the few fields it reads) and leaves a row in a tile per selected plane, and the
 * wave writes those out as it fetched. LDS is sized by the launch: a tile for the input and one per selected plane, 4 352 bytes
 * each, so two planes leave twelve waves to a CU and all six five. The same kernel walks a round's list of chunks again.
 *
 * nfc_tap_seam_kernel, a thread per chunk, finds per buffer the first chunk behind the true ones that did not start where the
 * one before it ended (a minimum over the buffer: a vector atomic in memory); nfc_tap_list_kernel, a thread per buffer, moves
 * the buffer's frontier there and lists the chunk. The host reads the length of the list, one word per round.
 */
#include <hip/hip_runtime.h>

#define NFC_DEV __device__ __forceinline__
#define NFC_ATOMIC_ADD(ptr, value) atomicAdd((ptr), (value))
#define NFC_ANY(predicate) (__any(predicate) != 0)

#include "nfc_core.hpp"
#include "nfc_tap.hpp"

__global__ __launch_bounds__(64) void nfc_tap_walk_kernel(NfcTapArgs A, NfcConfig cfg)
{
   extern __shared__ float tiles[]; /* [1 + planes][64][17] */
   __shared__ NfcTapWalker walkers[NfcTapShape::kWalkers];

   float *tileIn = tiles, *tileOut = tiles + NfcTapShape::kPlaneFloats;

   const uint32_t lane = threadIdx.x;
   const uint32_t planes = nfc_tap_planes(A.mask);
   const uint64_t groups = (A.walkers + NfcTapShape::kWalkers - 1) / NfcTapShape::kWalkers;

   for (uint64_t group = blockIdx.x; group < groups; group += gridDim.x)
   {
      const NfcTapWalker w = nfc_tap_walker(A, group * NfcTapShape::kWalkers + lane);

      walkers[lane] = w;

      NfcTapState s = w.total ? nfc_tap_begin(A, w) : nfc_tap_fresh();
      NfcTapState start = s;

      __syncthreads();

      for (uint32_t tile = 0; tile < A.tiles; tile++)
      {
         nfc_tap_fetch(A, walkers, tile, lane, tileIn);
         __syncthreads();
         nfc_tap_walk(A, cfg, w, tile, lane, s, start, tileIn, tileOut);
         __syncthreads();
         nfc_tap_store(A, walkers, tile, lane, planes, tileOut);
      }

      nfc_tap_end(A, w, start, s);
      __syncthreads();
   }
}

__global__ __launch_bounds__(256) void nfc_tap_seam_kernel(NfcTapArgs A)
{
   const uint64_t total = (uint64_t)A.nBuffers * A.chunksPerBuffer;

   for (uint64_t id = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; id < total; id += (uint64_t)gridDim.x * blockDim.x)
   {
      if (nfc_tap_seam_open(A, (uint32_t)id))
         atomicMin(&A.next[id / A.chunksPerBuffer], (uint32_t)(id % A.chunksPerBuffer));
   }
}

__global__ __launch_bounds__(256) void nfc_tap_list_kernel(NfcTapArgs A)
{
   for (uint32_t b = blockIdx.x * blockDim.x + threadIdx.x; b < A.nBuffers; b += gridDim.x * blockDim.x)
   {
      uint32_t id;

      if (nfc_tap_seam_close(A, b, id))
         A.listOut[atomicAdd(A.count, 1u)] = id;
   }
}

__global__ __launch_bounds__(256) void nfc_tap_finish_kernel(NfcTapArgs A)
{
   for (uint32_t b = blockIdx.x * blockDim.x + threadIdx.x; b < A.nBuffers; b += gridDim.x * blockDim.x)
      nfc_tap_finish(A, b);
}
