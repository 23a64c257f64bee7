/*
 * TEST INFRASTRUCTURE — recorder of the golden capture files of nfcgpu_record / nfcgpu_wav_write (tests/golden/record/).
 *
 * Writes a file of floats through the reference's hw::RecordDevice (compiled from the reference tree where it lies,
 * unmodified) the way SignalStorageTask::writeRadio does: opened for writing at a sample rate and a channel count,
 * SignalBuffers written one after the other, closed. The input goes out in pieces of 1000 samples and of 24 samples in
 * turn, so that the device's conversion block and its header rewrite on close see more than one write.
 *
 * No build script compiles this file: it is built by hand for a recording, with the command line written down in
 * tests/golden/record/README.md.
 *
 * usage: record-ref in.f32 out.wav channels [sample_rate]
 *   in.f32   float32 values; with channels = 2 interleaved I/Q
 *   out.wav  what hw::RecordDevice writes
 */
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <vector>

#include <rt/Logger.h>

#include <hw/RecordDevice.h>
#include <hw/SignalBuffer.h>
#include <hw/SignalType.h>

int main(int argc, char *argv[])
{
   if (argc < 4)
   {
      std::fprintf(stderr, "usage: %s in.f32 out.wav channels [sample_rate]\n", argv[0]);
      return 2;
   }

   const unsigned int channels = (unsigned int)std::atoi(argv[3]);
   const unsigned int sampleRate = argc > 4 ? (unsigned int)std::atoi(argv[4]) : 10000000;

   std::FILE *in = std::fopen(argv[1], "rb");

   if (!in || (channels != 1 && channels != 2))
   {
      std::fprintf(stderr, "cannot open %s, or channels is neither 1 nor 2\n", argv[1]);
      return 1;
   }

   std::vector<float> data;
   float value;

   while (std::fread(&value, sizeof(float), 1, in) == 1)
      data.push_back(value);

   std::fclose(in);

   rt::Logger::init(std::cerr);
   rt::Logger::setRootLevel(rt::Logger::WARN_LEVEL);

   hw::RecordDevice device {std::string(argv[2])};

   device.set(hw::SignalDevice::PARAM_SAMPLE_RATE, sampleRate, -1);
   device.set(hw::SignalDevice::PARAM_CHANNEL_COUNT, channels, -1);

   if (!device.open(hw::RecordDevice::Write))
   {
      std::fprintf(stderr, "cannot open %s for writing\n", argv[2]);
      return 1;
   }

   const size_t samples = data.size() / channels;
   size_t at = 0, written = 0;

   for (unsigned int piece = 0; at < samples; piece++)
   {
      size_t count = piece & 1 ? 24 : 1000;

      if (count > samples - at)
         count = samples - at;

      hw::SignalBuffer buffer(count * channels, channels, 1, sampleRate, at, 0,
                              channels == 2 ? hw::SignalType::SIGNAL_TYPE_RADIO_IQ : hw::SignalType::SIGNAL_TYPE_RADIO_SAMPLES, 0);

      buffer.put(data.data() + at * channels, count * channels).flip();

      if (device.write(buffer) < 0)
      {
         std::fprintf(stderr, "write failed at sample %zu\n", at);
         return 3;
      }

      at += count;
      written++;
   }

   device.close();

   std::printf("WROTE %zu samples x %u channels in %zu buffers\n", samples, channels, written);

   return 0;
}
