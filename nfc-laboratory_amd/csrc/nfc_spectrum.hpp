/*
 * nfc_spectrum.hpp - arithmetic of nfcgpu_spectrum, the spectrum the reference's FourierProcessTask publishes on "signal.fft"
 * (lab-tasks/src/main/cpp/tasks/FourierProcessTask.cpp:236-355), held once: the device kernels (nfc_spectrum.hip) and their
 * CPU twins of the emulated test build (nfcgpu.hip, NFCGPU_EMULATED_TEST_BUILD) compile this text.
 *
 * One workgroup transforms one frame of L complex points: L / 4 threads up to L = 1024 (one radix-4 butterfly per thread and pass,
 * four points in registers), 256 threads beyond (L / 256 points per thread).
 *
 *   step 0             gather the frame (FourierProcessTask.cpp:250-262: FFT input m is source pair 4 D (m >> 2) + (m & 3)),
 *                      float pairs or the int16 pairs of a capture file converted as they are loaded (nfc_sample.hpp),
 *                      one fp32 product with the window per component, first radix-4 pass (its twiddles are all 1)
 *   step 2 q - 1       results of pass q - 1 to LDS at their Stockham positions
 *   step 2 q           inputs of pass q from LDS (consecutive lanes read consecutive points), twiddles, butterflies
 *   last step          sqrtf(re * re + im * im), products and sum rounded separately (:279-341), stored with the halves
 *                      swapped (:344-348: negative frequencies first)
 *
 * Passes are radix 4, with one closing radix-2 pass when log2 L is odd. A step is a function of (frame, thread); whoever calls
 * the steps puts a barrier between them. The transform is the autosort form: pass q with p = 4^q combines, for thread i of L / R,
 * k = i mod p, the points i + r L / R (r < R) turned by W^(k r L / (p R)) and leaves them at (i - k) R + k + r p, so the last
 * pass ends in natural order and nothing is bit-reversed.
 *
 * LDS holds real and imaginary parts in two float arrays, index n kept at n + n / 32. Reads are contiguous over the lanes. The
 * stores of the first pass (stride 4 over the lanes) fall on 32 different banks per group of 32 lanes that way; those of the
 * passes with p = 4 and p = 16 are two-way, which a 4-byte LDS store does not pay for; from p = 64 on they are contiguous.
 *
 * Twiddles and window come from tables the host computes (nfcgpu.hip: spectrum_tables): nothing here depends on the device's
 * approximations, and with contraction off (the build's flag) the twin and the device do the same fp32 operations in the same
 * order for every output.
 */
#ifndef NFC_SPECTRUM_HPP
#define NFC_SPECTRUM_HPP

#include <stdint.h>

#include "nfc_sample.hpp"

struct NfcSpectrumArgs
{
   const float2 *iq;        /* buffer b starts at iq + b * inPitchPairs; int16 input: NfcIq16 pairs behind this pointer */
   float *out;              /* frame f of buffer b: out + b * outPitchFloats + f * L */
   const float *window;     /* L factors */
   const float2 *twiddle;   /* L entries: exp(-2 pi i n / L), computed in double, rounded to float */
   uint64_t inPitchPairs;
   uint64_t outPitchFloats;
   uint64_t total;          /* nBuffers * frames */
   uint32_t frames;         /* per buffer */
   uint32_t hop;            /* pairs between the starts of successive frames */
   uint32_t decimation;
};

#ifdef NFCGPU_EMULATED_TEST_BUILD
/* (the test build has no FMA and is compiled without contraction: the plain operators are the rounded ones) */
static inline float nfc_spec_mul(float a, float b) { return a * b; }
static inline float nfc_spec_add(float a, float b) { return a + b; }
static inline float nfc_spec_sqrt(float a) { return __builtin_sqrtf(a); }
#else
static __device__ __forceinline__ float nfc_spec_mul(float a, float b) { return __fmul_rn(a, b); }
static __device__ __forceinline__ float nfc_spec_add(float a, float b) { return __fadd_rn(a, b); }
/* (the correctly rounded root, as nfc_iq_magnitude takes it: __fsqrt_rn compiles to the bare v_sqrt_f32, which is within one unit
 * in the last place and not the reference's sqrtf) */
static __device__ __forceinline__ float nfc_spec_sqrt(float a) { return __builtin_sqrtf(a); }
#endif

template <int L>
struct NfcSpectrumShape
{
   static constexpr int log2Length()
   {
      int n = 0;
      for (int v = L; v > 1; v >>= 1)
         n++;
      return n;
   }
   static constexpr int kLog2 = log2Length();
   static constexpr int kPasses4 = kLog2 / 2;
   static constexpr int kPasses = kPasses4 + (kLog2 & 1);
   static constexpr int kSteps = 2 * kPasses;
   static constexpr int kThreads = L / 4 < 256 ? L / 4 : 256;  /* per frame: one radix-4 butterfly per thread and pass up to L = 1024 */
   static constexpr int kPoints = L / kThreads;                /* per thread */
   static constexpr int kLdsFloats = L + L / 32;               /* per component */
   static constexpr int radix(int pass) { return pass < kPasses4 ? 4 : 2; }
   static constexpr int span(int pass) { return 1 << (2 * pass); } /* p: product of the radices of the passes before */

   static_assert(L >= 256 && L <= 4096 && (L & (L - 1)) == 0, "FFT length: a power of two, 256 ... 4096");
};

template <int L>
struct NfcSpectrumRegs
{
   float re[NfcSpectrumShape<L>::kPoints], im[NfcSpectrumShape<L>::kPoints];
};

static __device__ __forceinline__ int nfc_spec_slot(int n) { return n + (n >> 5); }

/* forward butterfly of R points in place (R = 4 or 2) */
template <int R>
static __device__ __forceinline__ void nfc_spec_butterfly(float *re, float *im)
{
   if constexpr (R == 4)
   {
      const float ar = re[0] + re[2], ai = im[0] + im[2];
      const float br = re[0] - re[2], bi = im[0] - im[2];
      const float cr = re[1] + re[3], ci = im[1] + im[3];
      const float dr = re[1] - re[3], di = im[1] - im[3];
      /* -i (d) = (di, -dr) */
      re[0] = ar + cr; im[0] = ai + ci;
      re[1] = br + di; im[1] = bi - dr;
      re[2] = ar - cr; im[2] = ai - ci;
      re[3] = br - di; im[3] = bi + dr;
   }
   else
   {
      const float ar = re[0] + re[1], ai = im[0] + im[1];
      const float br = re[0] - re[1], bi = im[0] - im[1];
      re[0] = ar; im[0] = ai;
      re[1] = br; im[1] = bi;
   }
}

/* a source pair as two floats: the pair as it lies (float input), or an int16 pair - one 32-bit load - with both components
 * converted (nfc_i16_to_float, exact). The kernels exist once per format. */
static __device__ __forceinline__ float2 nfc_spectrum_pair(float2 v) { return v; }
static __device__ __forceinline__ float2 nfc_spectrum_pair(NfcIq16 v)
{
   float2 pair;
   pair.x = nfc_i16_to_float(v.i);
   pair.y = nfc_i16_to_float(v.q);
   return pair;
}

template <bool I16> struct NfcSpectrumSource { typedef float2 Pair; };
template <> struct NfcSpectrumSource<true> { typedef NfcIq16 Pair; };

/* step 0: gather, window, first pass */
template <int L, bool I16>
static __device__ __forceinline__ void nfc_spectrum_load(const NfcSpectrumArgs &A, uint64_t frame, int lane, NfcSpectrumRegs<L> &regs)
{
   constexpr int T = L / 4, NT = NfcSpectrumShape<L>::kThreads;
   const uint64_t buffer = frame / A.frames, f = frame % A.frames;
   const typename NfcSpectrumSource<I16>::Pair *src = reinterpret_cast<const typename NfcSpectrumSource<I16>::Pair *>(A.iq) + buffer * A.inPitchPairs + f * A.hop;
   const uint64_t group = 4ull * A.decimation;

#pragma unroll
   for (int b = 0; b < T / NT; b++)
   {
      const int i = lane + NT * b;
      float re[4], im[4];

#pragma unroll
      for (int r = 0; r < 4; r++)
      {
         const int m = i + r * T;
         const float2 v = nfc_spectrum_pair(src[group * (uint64_t)(m >> 2) + (uint64_t)(m & 3)]);
         const float w = A.window[m];
         re[r] = nfc_spec_mul(v.x, w);
         im[r] = nfc_spec_mul(v.y, w);
      }

      nfc_spec_butterfly<4>(re, im);

#pragma unroll
      for (int r = 0; r < 4; r++)
      {
         regs.re[4 * b + r] = re[r];
         regs.im[4 * b + r] = im[r];
      }
   }
}

/* step 2 q - 1 (PASS = q - 1): what pass PASS left in the registers goes to its place in LDS */
template <int L, int PASS>
static __device__ __forceinline__ void nfc_spectrum_scatter(int lane, const NfcSpectrumRegs<L> &regs, float *ldsRe, float *ldsIm)
{
   constexpr int R = NfcSpectrumShape<L>::radix(PASS), p = NfcSpectrumShape<L>::span(PASS), T = L / R, NT = NfcSpectrumShape<L>::kThreads;

#pragma unroll
   for (int b = 0; b < T / NT; b++)
   {
      const int i = lane + NT * b;
      const int k = i & (p - 1);
      const int j = (i - k) * R + k;

#pragma unroll
      for (int r = 0; r < R; r++)
      {
         const int slot = nfc_spec_slot(j + r * p);
         ldsRe[slot] = regs.re[R * b + r];
         ldsIm[slot] = regs.im[R * b + r];
      }
   }
}

/* step 2 q (PASS = q >= 1): inputs from LDS, twiddles, butterflies */
template <int L, int PASS>
static __device__ __forceinline__ void nfc_spectrum_gather(const NfcSpectrumArgs &A, int lane, NfcSpectrumRegs<L> &regs, const float *ldsRe,
                                                           const float *ldsIm)
{
   constexpr int R = NfcSpectrumShape<L>::radix(PASS), p = NfcSpectrumShape<L>::span(PASS), T = L / R, NT = NfcSpectrumShape<L>::kThreads;
   constexpr int step = L / (p * R); /* W_(pR)^(k r) = table[k r step] */

#pragma unroll
   for (int b = 0; b < T / NT; b++)
   {
      const int i = lane + NT * b;
      const int k = i & (p - 1);
      float re[R], im[R];

#pragma unroll
      for (int r = 0; r < R; r++)
      {
         const int slot = nfc_spec_slot(i + r * T);
         const float xr = ldsRe[slot], xi = ldsIm[slot];

         if (r == 0)
         {
            re[r] = xr;
            im[r] = xi;
         }
         else
         {
            const float2 w = A.twiddle[k * r * step];
            re[r] = xr * w.x - xi * w.y;
            im[r] = xr * w.y + xi * w.x;
         }
      }

      nfc_spec_butterfly<R>(re, im);

#pragma unroll
      for (int r = 0; r < R; r++)
      {
         regs.re[R * b + r] = re[r];
         regs.im[R * b + r] = im[r];
      }
   }
}

/* last step: the last pass leaves bin i + r T in register R b + r; output index = bin + L / 2 mod L */
template <int L>
static __device__ __forceinline__ void nfc_spectrum_store(const NfcSpectrumArgs &A, uint64_t frame, int lane, const NfcSpectrumRegs<L> &regs)
{
   constexpr int R = NfcSpectrumShape<L>::radix(NfcSpectrumShape<L>::kPasses - 1), T = L / R, NT = NfcSpectrumShape<L>::kThreads;
   const uint64_t buffer = frame / A.frames, f = frame % A.frames;
   float *dst = A.out + buffer * A.outPitchFloats + f * (uint64_t)L;

#pragma unroll
   for (int b = 0; b < T / NT; b++)
   {
#pragma unroll
      for (int r = 0; r < R; r++)
      {
         const int bin = lane + NT * b + r * T;
         const float x = regs.re[R * b + r], y = regs.im[R * b + r];
         dst[(bin + L / 2) & (L - 1)] = nfc_spec_sqrt(nfc_spec_add(nfc_spec_mul(x, x), nfc_spec_mul(y, y)));
      }
   }
}

/* step STEP of NfcSpectrumShape<L>::kSteps for thread `lane` of the workgroup that owns `frame`; a barrier belongs between two steps.
 * I16: the input is int16 pairs; only step 0 knows. */
template <int L, int STEP, bool I16 = false>
static __device__ __forceinline__ void nfc_spectrum_step(const NfcSpectrumArgs &A, uint64_t frame, int lane, NfcSpectrumRegs<L> &regs, float *ldsRe,
                                                         float *ldsIm)
{
   if constexpr (STEP == 0)
      nfc_spectrum_load<L, I16>(A, frame, lane, regs);
   else if constexpr (STEP == NfcSpectrumShape<L>::kSteps - 1)
      nfc_spectrum_store<L>(A, frame, lane, regs);
   else if constexpr (STEP & 1)
      nfc_spectrum_scatter<L, (STEP - 1) / 2>(lane, regs, ldsRe, ldsIm);
   else
      nfc_spectrum_gather<L, STEP / 2>(A, lane, regs, ldsRe, ldsIm);
}

#endif
