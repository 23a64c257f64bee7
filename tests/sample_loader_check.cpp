/* TEST INFRASTRUCTURE. The decoder's sample loader (nfc-laboratory_amd/csrc/nfc_sample.hpp: the text the kernels compile) on the
 * host: every sample of a file of raw samples in the given layout, through nfc_sample_at, written as raw floats.
 * tests/test_sample_loader.py compares the result with numpy, value by value.
 *    sample_loader_check <layout: 1, 2 float magnitude / IQ; 257, 258 int16 magnitude / IQ> <in> <out> */
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "nfc_sample.hpp"

int main(int argc, char **argv)
{
   if (argc != 4)
      return 2;

   const uint32_t layout = (uint32_t)std::strtoul(argv[1], nullptr, 10);
   const uint32_t components = nfc_sample_components(layout);

   if ((components != 1 && components != 2) || (layout & ~(0xFFu | NFC_SAMPLE_I16)))
      return 2;

   FILE *in = std::fopen(argv[2], "rb");
   if (!in)
      return 3;

   std::fseek(in, 0, SEEK_END);
   const long bytes = std::ftell(in);
   std::fseek(in, 0, SEEK_SET);

   /* (8-byte aligned, as rows of float IQ have to be) */
   std::vector<uint64_t> raw((size_t)bytes / 8 + 1);
   if (std::fread(raw.data(), 1, (size_t)bytes, in) != (size_t)bytes)
      return 3;
   std::fclose(in);

   const size_t n = (size_t)bytes / nfc_sample_bytes(layout);
   std::vector<float> out(n);

   for (size_t i = 0; i < n; i++)
      out[i] = nfc_sample_at((const uint8_t *)raw.data(), layout, (uint32_t)i);

   FILE *to = std::fopen(argv[3], "wb");
   if (!to || std::fwrite(out.data(), 4, n, to) != n)
      return 4;
   std::fclose(to);

   std::printf("%zu samples of %u bytes\n", n, nfc_sample_bytes(layout));
   return 0;
}
