/*
 * TEST INFRASTRUCTURE - the yardstick of nfcgpu_signal_tap (tests/test_signal_tap.py): the device step machine's front end
 * compiled for the CPU and walked over a buffer in one scalar loop, no chunks - per sample ++clock, ++pulseFilter,
 * nfc_front_end_core (nfc-laboratory_amd/csrc/nfc_core.hpp), and the depth as nfc_front_end forms it. Nothing of the tap's own
 * code (nfc_tap.hpp) is compiled here.
 *
 * usage: tap_walk_check sample_rate in.f32 state_in.bin planes.f32 state_out.bin
 *   in.f32         n float32 samples (magnitudes)
 *   state_in.bin   32 bytes: clock, pulse filter (uint32), envelope, filter, deviation, average (float32), 8 bytes unused
 *   planes.f32     six planes of n float32: value, filtered, deviation, average, envelope, depth
 *   state_out.bin  32 bytes: the state behind the last sample
 * Built by the test with g++ -O2 -ffp-contract=off -msse3 -mno-avx, the flags of the other CPU builds of this text.
 */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define NFC_DEV static inline
static inline uint32_t check_add(uint32_t *p, uint32_t v) { const uint32_t old = *p; *p += v; return old; }
#define NFC_ATOMIC_ADD(ptr, value) check_add((ptr), (value))
#define NFC_ANY(predicate) (predicate)

#include "nfc_core.hpp"
#include "nfc_config.hpp"

struct State
{
   uint32_t clock, pulseFilter;
   float env, n1, mdev, avg;
   uint32_t reserved[2];
};

int main(int argc, char *argv[])
{
   if (argc != 6)
   {
      std::fprintf(stderr, "usage: %s sample_rate in.f32 state_in.bin planes.f32 state_out.bin\n", argv[0]);
      return 2;
   }

   NfcHostParams hp;
   static NfcConfig cfg;
   hp.sampleRate = (uint32_t)std::strtoul(argv[1], nullptr, 10);

   if (!nfc_build_config(hp, cfg))
   {
      std::fprintf(stderr, "sample rate %s is not decodable\n", argv[1]);
      return 1;
   }

   std::vector<float> x;
   State st;
   std::FILE *f = std::fopen(argv[2], "rb");

   if (!f)
      return 1;

   float value;
   while (std::fread(&value, sizeof(float), 1, f) == 1)
      x.push_back(value);
   std::fclose(f);

   f = std::fopen(argv[3], "rb");
   if (!f || std::fread(&st, sizeof(st), 1, f) != 1)
      return 1;
   std::fclose(f);

   static NfcStreamState s;
   std::memset(&s, 0, sizeof(s));
   s.clock = st.clock; s.pulseFilter = st.pulseFilter;
   s.env = st.env; s.n1 = st.n1; s.mdev = st.mdev; s.avg = st.avg;

   const size_t n = x.size();
   std::vector<float> planes(6 * n);

   for (size_t i = 0; i < n; i++)
   {
      ++s.clock;
      ++s.pulseFilter;

      const NfcNow now = nfc_front_end_core(cfg, s, x[i]);

      const float env = s.env;
      const float clamped = (x[i] < 0.0f) ? 0.0f : ((env < x[i]) ? env : x[i]);

      planes[0 * n + i] = now.x;
      planes[1 * n + i] = now.filt;
      planes[2 * n + i] = now.mdev;
      planes[3 * n + i] = s.avg;
      planes[4 * n + i] = env;
      planes[5 * n + i] = (env - clamped) / env;
   }

   std::memset(&st, 0, sizeof(st));
   st.clock = s.clock; st.pulseFilter = s.pulseFilter;
   st.env = s.env; st.n1 = s.n1; st.mdev = s.mdev; st.avg = s.avg;

   f = std::fopen(argv[4], "wb");
   if (!f || (n && std::fwrite(planes.data(), sizeof(float), planes.size(), f) != planes.size()))
      return 1;
   std::fclose(f);

   f = std::fopen(argv[5], "wb");
   if (!f || std::fwrite(&st, sizeof(st), 1, f) != 1)
      return 1;
   std::fclose(f);

   return 0;
}
