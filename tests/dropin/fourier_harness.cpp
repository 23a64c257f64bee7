/*
 * TEST INFRASTRUCTURE — recorder of the golden vectors of nfcgpu_spectrum (tests/golden/spectrum/fourier_task.npy).
 *
 * Runs the reference's lab::FourierProcessTask (compiled from the reference tree where it lies, unmodified, with the
 * -msse2 -DUSE_SSE2 of lab-tasks/CMakeLists.txt:18 and the reference's vendored mufft) the way the application does:
 * submitted to an rt::Executor, one SIGNAL_TYPE_RADIO_IQ buffer published on "radio.signal.iq", enabled through
 * "fourier.command" ({"enabled": true}), the first buffer it publishes on "signal.fft" taken. The task transforms
 * whatever buffer arrived last every 10 ms, so every later buffer on "signal.fft" repeats the first; it is switched off
 * again before the next input is published.
 *
 * No build script compiles this file: it is built by hand for a recording, with the command line written down in
 * tests/golden/spectrum/README.md.
 *
 * usage: fourier-ref in.f32 out.f32 [pairs_per_buffer] [sample_rate]
 *   in.f32   interleaved float32 IQ, one buffer of pairs_per_buffer (16384) pairs after the other
 *   out.f32  per input buffer the floats of the published buffer (1024: negative frequencies first)
 * prints "BUFFER <index> <floats> type <type> rate <sample rate> decimation <decimation>" per buffer.
 */
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <mutex>
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

#include <lab/tasks/FourierProcessTask.h>

using json = nlohmann::json;

namespace {

bool command(rt::Subject<rt::Event> *subject, int code, const json &data)
{
   std::atomic<int> outcome {0};

   subject->next({code, [&outcome] { outcome = 1; }, [&outcome](int, const std::string &) { outcome = -1; }, {{"data", data.dump()}}});

   for (int i = 0; i < 2000 && outcome == 0; i++)
      std::this_thread::sleep_for(std::chrono::milliseconds(5));

   return outcome == 1;
}

}

int main(int argc, char *argv[])
{
   if (argc < 3)
   {
      std::fprintf(stderr, "usage: %s in.f32 out.f32 [pairs_per_buffer] [sample_rate]\n", argv[0]);
      return 2;
   }

   const unsigned int pairs = argc > 3 ? (unsigned int)std::atoi(argv[3]) : 16384;
   const unsigned int sampleRate = argc > 4 ? (unsigned int)std::atoi(argv[4]) : 10000000;

   std::FILE *in = std::fopen(argv[1], "rb");
   std::FILE *out = std::fopen(argv[2], "wb");

   if (!in || !out)
   {
      std::fprintf(stderr, "cannot open %s or %s\n", argv[1], argv[2]);
      return 1;
   }

   rt::Logger::init(std::cerr);
   rt::Logger::setRootLevel(rt::Logger::WARN_LEVEL);

   int status = 0;

   {
      rt::Executor executor(16, 4);

      executor.submit(lab::FourierProcessTask::construct());

      auto *commands = rt::Subject<rt::Event>::name("fourier.command");
      auto *signal = rt::Subject<hw::SignalBuffer>::name("radio.signal.iq");
      auto *spectrum = rt::Subject<hw::SignalBuffer>::name("signal.fft");

      std::mutex lock;
      std::vector<float> first;
      unsigned int type = 0, rate = 0, decimation = 0;
      std::atomic<bool> taken {true};

      auto subscription = spectrum->subscribe([&](const hw::SignalBuffer &buffer) {
         if (taken || !buffer.isValid())
            return;

         std::lock_guard<std::mutex> guard(lock);
         first.assign(buffer.data(), buffer.data() + buffer.limit());
         type = buffer.type();
         rate = buffer.sampleRate();
         decimation = buffer.decimation();
         taken = true;
      });

      /* the worker starts on a thread of the executor: give start() the time to fill the window table */
      std::this_thread::sleep_for(std::chrono::milliseconds(200));

      std::vector<float> data(2 * (size_t)pairs);

      for (unsigned int index = 0; std::fread(data.data(), sizeof(float), data.size(), in) == data.size(); index++)
      {
         hw::SignalBuffer samples(2 * pairs, 2, 1, sampleRate, 0, 0, hw::SignalType::SIGNAL_TYPE_RADIO_IQ, 0);

         samples.put(data.data(), data.size()).flip();
         signal->next(samples);

         taken = false;

         if (!command(commands, lab::FourierProcessTask::Configure, {{"enabled", true}}))
         {
            status = 3;
            break;
         }

         for (int i = 0; i < 2000 && !taken; i++)
            std::this_thread::sleep_for(std::chrono::milliseconds(5));

         if (!taken)
         {
            std::fprintf(stderr, "buffer %u: nothing on signal.fft\n", index);
            status = 4;
            break;
         }

         /* once this is resolved the task's loop no longer calls process() */
         if (!command(commands, lab::FourierProcessTask::Configure, {{"enabled", false}}))
         {
            status = 3;
            break;
         }

         std::lock_guard<std::mutex> guard(lock);
         std::fwrite(first.data(), sizeof(float), first.size(), out);
         std::printf("BUFFER %u %zu type %u rate %u decimation %u\n", index, first.size(), type, rate, decimation);
      }

      executor.shutdown();
   }

   std::fclose(in);
   std::fclose(out);

   return status;
}
