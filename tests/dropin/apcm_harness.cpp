/*
 * TEST INFRASTRUCTURE - how the golden traces of tests/golden/apcm/ were made (see the README there). Compiled by no script.
 *
 * Runs the reference's lab::SignalResamplingTask and lab::TraceStorageTask (compiled from the reference tree where it lies,
 * unmodified) the way the application does: both submitted to an rt::Executor, SIGNAL_TYPE_RADIO_SAMPLES buffers published on
 * "radio.signal.raw", the resampler's control points taken by the trace task from "adaptive.signal", then "write file"
 * (storage.command Write) with a time range. The trace holds frame.json (no frames) and radio-0.apcm as the reference writes it.
 *
 * usage: apcm-ref in.f32 samples_per_buffer sample_rate out.trz time_start time_end
 *   in.f32: float32 magnitudes; they are published in buffers of samples_per_buffer with id 0 and the offsets j * samples_per_buffer.
 */
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <string>
#include <thread>
#include <vector>

#include <nlohmann/json.hpp>

#include <rt/Event.h>
#include <rt/Executor.h>
#include <rt/Logger.h>
#include <rt/Subject.h>

#include <hw/SignalBuffer.h>
#include <hw/SignalType.h>

#include <lab/tasks/SignalResamplingTask.h>
#include <lab/tasks/TraceStorageTask.h>

using json = nlohmann::json;

int main(int argc, char *argv[])
{
   if (argc < 7)
   {
      std::fprintf(stderr, "usage: %s in.f32 samples_per_buffer sample_rate out.trz time_start time_end\n", argv[0]);
      return 2;
   }

   const unsigned int perBuffer = (unsigned int)std::atoi(argv[2]);
   const unsigned int sampleRate = (unsigned int)std::atoi(argv[3]);
   const double timeStart = std::atof(argv[5]), timeEnd = std::atof(argv[6]);

   std::vector<float> samples;

   if (std::FILE *in = std::fopen(argv[1], "rb"))
   {
      float block[4096];
      size_t got;
      while ((got = std::fread(block, sizeof(float), 4096, in)) > 0)
         samples.insert(samples.end(), block, block + got);
      std::fclose(in);
   }

   if (samples.empty() || perBuffer == 0 || samples.size() % perBuffer != 0)
   {
      std::fprintf(stderr, "no samples, or not whole buffers\n");
      return 2;
   }

   rt::Logger::init(std::cerr);
   rt::Logger::setRootLevel(rt::Logger::WARN_LEVEL);

   int status = 0;

   {
      rt::Executor executor(16, 4);

      executor.submit(lab::SignalResamplingTask::construct());
      executor.submit(lab::TraceStorageTask::construct());

      auto *signal = rt::Subject<hw::SignalBuffer>::name("radio.signal.raw");
      auto *adaptive = rt::Subject<hw::SignalBuffer>::name("adaptive.signal");
      auto *commands = rt::Subject<rt::Event>::name("storage.command");

      std::atomic<unsigned int> resampled {0};

      auto subscription = adaptive->subscribe([&](const hw::SignalBuffer &buffer) {
         if (buffer.isValid())
            resampled++;
      });

      std::this_thread::sleep_for(std::chrono::milliseconds(200));

      const unsigned int buffers = (unsigned int)(samples.size() / perBuffer);

      for (unsigned int j = 0; j < buffers; j++)
      {
         hw::SignalBuffer buffer(perBuffer, 1, 1, sampleRate, (unsigned long long)j * perBuffer, 0, hw::SignalType::SIGNAL_TYPE_RADIO_SAMPLES, 0);

         buffer.put(samples.data() + (size_t)j * perBuffer, perBuffer).flip();
         signal->next(buffer);
      }

      for (int i = 0; i < 12000 && resampled < buffers; i++)
         std::this_thread::sleep_for(std::chrono::milliseconds(5));

      /* (the trace task takes a buffer in the same notification: a moment for its queue) */
      std::this_thread::sleep_for(std::chrono::milliseconds(200));

      if (resampled < buffers)
         status = 3;
      else
      {
         std::atomic<int> outcome {0};
         const json data = {{"fileName", argv[4]}, {"timeStart", timeStart}, {"timeEnd", timeEnd}};

         commands->next({lab::TraceStorageTask::Write, [&outcome] { outcome = 1; }, [&outcome](int, const std::string &) { outcome = -1; }, {{"data", data.dump()}}});

         for (int i = 0; i < 12000 && outcome == 0; i++)
            std::this_thread::sleep_for(std::chrono::milliseconds(5));

         if (outcome != 1)
            status = 4;
      }

      executor.shutdown();
   }

   std::printf("DONE %s status %d\n", argv[4], status);

   return status;
}
