/*
 * nfc_trace.hip — trace (.trz) writer behind the C ABI: decoded frames in the on-disk format the
 * reference application opens ("open trace") and tools/py_nfclab reads, so that what a GPU run decodes can be inspected
 * with the reference's own tools. Host code only (no kernel in this file).
 *
 * Format, as the reference's TraceStorageTask writes and reads it (lab-tasks/src/main/cpp/tasks/TraceStorageTask.cpp:
 * writeFrameEntry 461-520, readFrameEntry 380-449, the time range of writeFile 211-240): a gzip-compressed tar archive
 * with one entry "frame.json" = {"frames":[{...},...]}, per frame sampleStart, sampleEnd, sampleRate, timeStart, timeEnd,
 * techType, frameType, frameRate, frameFlags, framePhase, dateTime and, for frames with payload, frameData ("26",
 * "04:00": upper-case hex bytes separated by colons) and length. Times follow the decoder: timeStart = sampleStart /
 * sampleRate, dateTime = streamTime + timeStart (NfcA.cpp frame construction, NfcDecoder.cpp:449-463); a range
 * [rangeStart, rangeEnd] keeps the frames inside it and shifts their times and sample numbers to its start
 * (TraceStorageTask.cpp:461-483).
 *
 * The signal goes into the same archive behind frame.json as entries "radio-<id>.apcm", one per stream, in the order and under the
 * names of writeTraceFile / writeRadioData (:322-364, :1032-1057): nfcgpu_trace_write_signal takes them as nfcgpu_apcm_encode made
 * them (nfc_apcm.hpp) and admits what the reference's reader admits (readRadioEntry :789-827).
 *
 * The archive is written without a compression library: per entry a ustar header + the entry, then two zero blocks, wrapped in a
 * gzip member whose deflate stream consists of stored blocks (RFC 1951 3.2.4) - any inflate reads it, the reference's included.
 */
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/nfcgpu.h"

namespace {

/* shortest decimal form that reads back as the same double (what nlohmann::json's dump and Python's repr give) */
void append_double(std::string &out, double v)
{
   char buf[40];

   for (int digits = 1; digits <= 17; digits++)
   {
      std::snprintf(buf, sizeof(buf), "%.*g", digits, v);

      double back = 0;
      if (std::sscanf(buf, "%lf", &back) == 1 && back == v)
         break;
   }

   out += buf;

   /* a JSON number that is a double keeps its fraction ("2.0", as the reference's writer prints it) */
   if (!std::strpbrk(buf, ".eEn"))
      out += ".0";
}

void append_uint(std::string &out, uint64_t v)
{
   char buf[24];
   std::snprintf(buf, sizeof(buf), "%llu", (unsigned long long)v);
   out += buf;
}

/* the table of CRC-32 (reflected 0xEDB88320), built once: a function-local static of class type is initialised exactly once
 * whatever threads call first (nfcgpu_trace_write_frames needs no context and may be called from several at a time) */
struct Crc32Table
{
   uint32_t entry[256];

   Crc32Table()
   {
      for (uint32_t i = 0; i < 256; i++)
      {
         uint32_t c = i;
         for (int k = 0; k < 8; k++)
            c = (c & 1u) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
         entry[i] = c;
      }
   }
};

uint32_t crc32_of(const uint8_t *p, size_t n)
{
   static const Crc32Table table;

   uint32_t c = 0xFFFFFFFFu;
   for (size_t i = 0; i < n; i++)
      c = table.entry[(c ^ p[i]) & 0xFFu] ^ (c >> 8);
   return c ^ 0xFFFFFFFFu;
}

/* one ustar entry (name, 0664, regular file) behind what the archive holds already */
void tar_add(std::vector<uint8_t> &tar, const char *name, const void *content, size_t size)
{
   const size_t at = tar.size();

   tar.resize(at + 512, 0);
   uint8_t *h = tar.data() + at;

   std::snprintf((char *)h, 100, "%s", name);
   std::snprintf((char *)h + 100, 8, "%07o", 0664);
   std::snprintf((char *)h + 108, 8, "%07o", 0);
   std::snprintf((char *)h + 116, 8, "%07o", 0);
   std::snprintf((char *)h + 124, 12, "%011llo", (unsigned long long)size);
   std::snprintf((char *)h + 136, 12, "%011o", 0);
   std::memset(h + 148, ' ', 8);
   h[156] = '0';
   std::memcpy(h + 257, "ustar", 6);
   h[263] = '0';
   h[264] = '0';

   unsigned sum = 0;
   for (int i = 0; i < 512; i++)
      sum += h[i];
   std::snprintf((char *)h + 148, 8, "%06o", sum);
   h[154] = 0;
   h[155] = ' ';

   tar.insert(tar.end(), (const uint8_t *)content, (const uint8_t *)content + size);
   tar.resize((tar.size() + 511) / 512 * 512, 0);
}

/* the archive's end marker */
void tar_end(std::vector<uint8_t> &tar)
{
   tar.resize(tar.size() + 1024, 0);
}

int write_gzip_stored(const char *path, const std::vector<uint8_t> &raw)
{
   std::FILE *f = std::fopen(path, "wb");
   if (!f)
      return NFCGPU_EIO;

   const uint8_t head[10] = {0x1F, 0x8B, 8, 0, 0, 0, 0, 0, 0, 0xFF};
   bool ok = std::fwrite(head, 1, sizeof(head), f) == sizeof(head);

   size_t at = 0;
   do
   {
      const size_t n = raw.size() - at < 65535 ? raw.size() - at : 65535;
      const bool last = at + n == raw.size();
      const uint8_t block[5] = {(uint8_t)(last ? 1 : 0), (uint8_t)(n & 0xFF), (uint8_t)(n >> 8), (uint8_t)(~n & 0xFF), (uint8_t)((~n >> 8) & 0xFF)};
      ok = ok && std::fwrite(block, 1, 5, f) == 5 && (n == 0 || std::fwrite(raw.data() + at, 1, n, f) == n);
      at += n;
   } while (at < raw.size());

   const uint32_t crc = crc32_of(raw.data(), raw.size());
   const uint32_t len = (uint32_t)raw.size();
   const uint8_t tail[8] = {(uint8_t)crc, (uint8_t)(crc >> 8), (uint8_t)(crc >> 16), (uint8_t)(crc >> 24), (uint8_t)len, (uint8_t)(len >> 8), (uint8_t)(len >> 16), (uint8_t)(len >> 24)};
   ok = ok && std::fwrite(tail, 1, 8, f) == 8;
   ok = (std::fclose(f) == 0) && ok;

   return ok ? NFCGPU_OK : NFCGPU_EIO;
}

/* frame.json of the frames inside the range (0, 0: all of them); *kept = how many */
std::string frames_json(const nfcgpu_frame *frames, uint32_t count, int64_t stream_time, double range_start, double range_end, uint32_t *keptOut)
{
   const bool ranged = range_end > range_start; /* (0, 0: everything) */
   std::string json = "{\"frames\":[";
   uint32_t kept = 0;

   for (uint32_t i = 0; i < count; i++)
   {
      const nfcgpu_frame &f = frames[i];
      const double rate = (double)f.sample_rate;
      const double timeStart = rate > 0 ? (double)f.sample_start / rate : 0.0;
      const double timeEnd = rate > 0 ? (double)f.sample_end / rate : 0.0;

      if (ranged && (timeStart < range_start || timeEnd > range_end))
         continue;

      const double shift = ranged ? range_start : 0.0;
      const uint64_t offset = ranged ? (uint64_t)((double)f.sample_rate * range_start) : 0u;

      if (kept++)
         json += ",";

      /* (keys in alphabetical order, as nlohmann::json's object prints them) */
      json += "{\"dateTime\":";
      append_double(json, (double)stream_time + timeStart);
      if (f.length)
      {
         json += ",\"frameData\":\"";
         for (uint32_t b = 0; b < f.length && b < sizeof(f.data); b++)
         {
            char hex[4];
            std::snprintf(hex, sizeof(hex), b ? ":%02X" : "%02X", f.data[b]);
            json += hex;
         }
         json += "\"";
      }
      json += ",\"frameFlags\":";
      append_uint(json, f.frame_flags);
      json += ",\"framePhase\":";
      append_uint(json, f.frame_phase);
      json += ",\"frameRate\":";
      append_uint(json, f.frame_rate);
      json += ",\"frameType\":";
      append_uint(json, f.frame_type);
      if (f.length)
      {
         json += ",\"length\":";
         append_uint(json, f.length < sizeof(f.data) ? f.length : (uint32_t)sizeof(f.data)); /* (the bytes frameData holds) */
      }
      json += ",\"sampleEnd\":";
      append_uint(json, f.sample_end - offset);
      json += ",\"sampleRate\":";
      append_uint(json, f.sample_rate);
      json += ",\"sampleStart\":";
      append_uint(json, f.sample_start - offset);
      json += ",\"techType\":";
      append_uint(json, f.tech_type);
      json += ",\"timeEnd\":";
      append_double(json, timeEnd - shift);
      json += ",\"timeStart\":";
      append_double(json, timeStart - shift);
      json += "}";
   }

   json += "]}";

   *keptOut = kept;
   return json;
}

uint32_t word_at(const uint8_t *at)
{
   return (uint32_t)at[0] | ((uint32_t)at[1] << 8) | ((uint32_t)at[2] << 16) | ((uint32_t)at[3] << 24);
}

}

extern "C" int nfcgpu_trace_write_frames(const char *path, const nfcgpu_frame *frames, uint32_t count, int64_t stream_time, double range_start, double range_end,
                                         uint32_t *written)
{
   return nfcgpu_trace_write_signal(path, frames, count, stream_time, range_start, range_end, written, nullptr, nullptr, 0);
}

/* frame.json, then the APCM entries as "radio-<id>.apcm" (TraceStorageTask.cpp:322-364, :1032-1057). An entry is taken when it is
 * what the reference's reader accepts (:789-827): the magic, version 2, a size of 32 + 3 * info[2]. */
extern "C" int nfcgpu_trace_write_signal(const char *path, const nfcgpu_frame *frames, uint32_t count, int64_t stream_time, double range_start, double range_end,
                                         uint32_t *written, const void *const *entries, const uint64_t *entry_bytes, uint32_t n_entries)
{
   if (!path || (count && !frames) || (n_entries && (!entries || !entry_bytes)))
      return NFCGPU_EINVAL;

   uint32_t kept = 0;
   const std::string json = frames_json(frames, count, stream_time, range_start, range_end, &kept);

   /* the archive's size and every header first: nothing of an entry's records is read before the archive is known to fit */
   auto blocks = [](uint64_t bytes) { return 512 + (bytes + 511) / 512 * 512; };
   uint64_t total = blocks(json.size()) + 1024;
   std::vector<uint32_t> ids(n_entries);

   for (uint32_t i = 0; i < n_entries; i++)
   {
      const uint8_t *e = (const uint8_t *)entries[i];

      if (!e || entry_bytes[i] < 32 || std::memcmp(e, "APCM", 4) != 0 || word_at(e + 4) != 2 || entry_bytes[i] != 32 + 3 * (uint64_t)word_at(e + 16))
         return NFCGPU_EINVAL;

      ids[i] = word_at(e + 20);

      for (uint32_t k = 0; k < i; k++)
         if (ids[k] == ids[i])
            return NFCGPU_EINVAL;

      total += blocks(entry_bytes[i]);

      if (total >= 0x100000000ull)
         return NFCGPU_EINVAL;
   }

   if (total >= 0x100000000ull)
      return NFCGPU_EINVAL;

   std::vector<uint8_t> tar;
   tar.reserve((size_t)total);
   tar_add(tar, "frame.json", json.data(), json.size());

   for (uint32_t i = 0; i < n_entries; i++)
   {
      char name[32];
      std::snprintf(name, sizeof(name), "radio-%u.apcm", ids[i]);
      tar_add(tar, name, entries[i], (size_t)entry_bytes[i]);
   }

   tar_end(tar);

   if (written)
      *written = kept;

   return write_gzip_stored(path, tar);
}

/* ---- capture files: the header hw::RecordDevice writes (RecordDevice.cpp:493-546, structures :53-100) and the samples behind it ---- */

namespace {

const uint32_t kWavHeaderBytes = 92;

void put16(uint8_t *at, uint32_t v)
{
   at[0] = (uint8_t)v;
   at[1] = (uint8_t)(v >> 8);
}

void put32(uint8_t *at, uint32_t v)
{
   put16(at, v);
   put16(at + 2, v >> 16);
}

uint32_t get16(const uint8_t *at)
{
   return (uint32_t)at[0] | ((uint32_t)at[1] << 8);
}

uint32_t get32(const uint8_t *at)
{
   return get16(at) | (get16(at + 2) << 16);
}

void wav_header(uint8_t *h, uint64_t fileBytes, uint32_t channels, uint32_t rate, uint32_t streamTime, const int32_t *keys)
{
   std::memset(h, 0, kWavHeaderBytes);
   std::memcpy(h, "RIFF", 4);
   put32(h + 4, (uint32_t)(fileBytes - 8));
   std::memcpy(h + 8, "WAVE", 4);
   std::memcpy(h + 12, "fmt ", 4);
   put32(h + 16, 16);
   put16(h + 20, 1);
   put16(h + 22, channels);
   put32(h + 24, rate);
   put32(h + 28, channels * rate * 2);
   put16(h + 32, channels * 2);
   put16(h + 34, 16);
   std::memcpy(h + 36, "META", 4);
   put32(h + 40, 40);
   std::memcpy(h + 44, "meta", 4);
   put32(h + 48, streamTime);
   for (uint32_t c = 0; keys && c < channels; c++)
      put32(h + 52 + 4 * c, (uint32_t)keys[c]);
   std::memcpy(h + 84, "data", 4);
   put32(h + 88, (uint32_t)(fileBytes - kWavHeaderBytes));
}

/* the channel count of a header of exactly that shape, or 0 */
uint32_t wav_header_channels(const uint8_t *h)
{
   if (std::memcmp(h, "RIFF", 4) || std::memcmp(h + 8, "WAVE", 4) || std::memcmp(h + 12, "fmt ", 4) || get32(h + 16) != 16 || get16(h + 20) != 1 ||
       get16(h + 34) != 16 || std::memcmp(h + 36, "META", 4) || get32(h + 40) != 40 || std::memcmp(h + 44, "meta", 4) || std::memcmp(h + 84, "data", 4))
      return 0;

   const uint32_t channels = get16(h + 22);

   if (channels == 0 || channels > 8 || get16(h + 32) != channels * 2)
      return 0;

   return channels;
}

bool wav_put_samples(std::FILE *f, const int16_t *pcm, uint64_t count)
{
   /* (little-endian samples, whatever the host) */
   std::vector<uint8_t> block(65536);

   while (count)
   {
      const size_t now = count < block.size() / 2 ? (size_t)count : block.size() / 2;
      for (size_t i = 0; i < now; i++)
         put16(block.data() + 2 * i, (uint16_t)pcm[i]);
      if (std::fwrite(block.data(), 2, now, f) != now)
         return false;
      pcm += now;
      count -= now;
   }

   return true;
}

}

extern "C" int nfcgpu_wav_write(const char *path, const int16_t *pcm, uint64_t n_samples, uint32_t channels, uint32_t sample_rate, uint32_t stream_time,
                                const int32_t *keys)
{
   if (!path || channels == 0 || channels > 8 || (n_samples && !pcm) || n_samples > (0xFFFFFFFFull - kWavHeaderBytes) / (2 * channels))
      return NFCGPU_EINVAL;

   std::FILE *f = std::fopen(path, "wb");
   if (!f)
      return NFCGPU_EIO;

   uint8_t header[kWavHeaderBytes];
   wav_header(header, kWavHeaderBytes + n_samples * channels * 2, channels, sample_rate, stream_time, keys);

   bool ok = std::fwrite(header, 1, kWavHeaderBytes, f) == kWavHeaderBytes && wav_put_samples(f, pcm, n_samples * channels);
   ok = (std::fclose(f) == 0) && ok;

   return ok ? NFCGPU_OK : NFCGPU_EIO;
}

extern "C" int nfcgpu_wav_append(const char *path, const int16_t *pcm, uint64_t n_samples)
{
   if (!path || (n_samples && !pcm))
      return NFCGPU_EINVAL;

   std::FILE *f = std::fopen(path, "r+b");
   if (!f)
      return NFCGPU_EIO;

   uint8_t header[kWavHeaderBytes];
   const bool whole = std::fread(header, 1, kWavHeaderBytes, f) == kWavHeaderBytes;
   const uint32_t channels = whole ? wav_header_channels(header) : 0;

   if (!channels || std::fseek(f, 0, SEEK_END) != 0)
   {
      std::fclose(f);
      return channels ? NFCGPU_EIO : NFCGPU_EINVAL;
   }

   const long at = std::ftell(f);
   const uint64_t length = at < 0 ? 0 : (uint64_t)at;

   if (length < kWavHeaderBytes || length != (uint64_t)get32(header + 88) + kWavHeaderBytes || length != (uint64_t)get32(header + 4) + 8 ||
       n_samples > (0xFFFFFFFFull - length) / (2 * channels))
   {
      std::fclose(f);
      return NFCGPU_EINVAL;
   }

   const uint64_t after = length + n_samples * channels * 2;
   bool ok = wav_put_samples(f, pcm, n_samples * channels);

   put32(header + 4, (uint32_t)(after - 8));
   put32(header + 88, (uint32_t)(after - kWavHeaderBytes));
   ok = ok && std::fseek(f, 0, SEEK_SET) == 0 && std::fwrite(header, 1, kWavHeaderBytes, f) == kWavHeaderBytes;
   ok = (std::fclose(f) == 0) && ok;

   return ok ? NFCGPU_OK : NFCGPU_EIO;
}
