/*
 * TEST INFRASTRUCTURE — recorder of the golden debug channels of nfcgpu_signal_tap (tests/golden/tap/).
 *
 * Drives the reference's lab::NfcDecoder (compiled from the reference tree where it lies, unmodified) with setEnableDebug(true)
 * over a file of float magnitudes, in buffers of 4099 samples, as a lab tool's user does who wants to see what the decoder
 * sees: NfcDecoderStatus::nextSample then hands every sample's values to NfcSignalDebug, which writes the ten-channel
 * radio-debug-<time>.wav into the working directory. The file is complete once the decoder is gone.
 *
 * No build script compiles this file: it is built by hand for a recording, with the command line written down in
 * tests/golden/tap/README.md.
 *
 * usage: tap-ref in.f32 [sample_rate]      (run in an empty directory; prints how much it fed)
 */
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <list>
#include <vector>

#include <rt/Logger.h>

#include <hw/SignalBuffer.h>
#include <hw/SignalType.h>

#include <lab/data/RawFrame.h>
#include <lab/nfc/NfcDecoder.h>

int main(int argc, char *argv[])
{
   if (argc < 2)
   {
      std::fprintf(stderr, "usage: %s in.f32 [sample_rate]\n", argv[0]);
      return 2;
   }

   const unsigned int sampleRate = argc > 2 ? (unsigned int)std::atoi(argv[2]) : 10000000;

   std::FILE *in = std::fopen(argv[1], "rb");

   if (!in)
   {
      std::fprintf(stderr, "cannot open %s\n", argv[1]);
      return 1;
   }

   std::vector<float> data;
   float value;

   while (std::fread(&value, sizeof(float), 1, in) == 1)
      data.push_back(value);

   std::fclose(in);

   rt::Logger::init(std::cerr);
   rt::Logger::setRootLevel(rt::Logger::WARN_LEVEL);

   size_t frames = 0, buffers = 0;

   {
      lab::NfcDecoder decoder;

      decoder.setEnableDebug(true);

      for (size_t at = 0; at < data.size(); at += 4099)
      {
         const size_t count = data.size() - at < 4099 ? data.size() - at : 4099;

         hw::SignalBuffer buffer(count, 1, 1, sampleRate, at, 0, hw::SignalType::SIGNAL_TYPE_RADIO_SAMPLES, 0);

         buffer.put(data.data() + at, count).flip();

         frames += decoder.nextFrames(buffer).size();
         buffers++;
      }
   }

   std::printf("FED %zu samples in %zu buffers, %zu frames\n", data.size(), buffers, frames);

   return 0;
}
