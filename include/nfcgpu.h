/*
 * nfcgpu.h — C ABI of libnfcgpu.so, the MI355X (gfx950) implementation of nfc-laboratory's radio
 * demodulation hot path. This is the drop-in boundary: everything above it (lab::NfcDecoder shim,
 * RadioDecoderTask, the Qt app, nfc-rx, test-sdr) is host C++ from the reference, unchanged.
 *
 * What each entry point replaces in the reference (paths relative to /root/reference/src/nfc-lib):
 *
 *   nfcgpu_init / nfcgpu_shutdown      process-wide decoder resources; the reference has none
 *                                      (lab::NfcDecoder::NfcDecoder(), lib-lab/lab-radio/src/main/cpp/NfcDecoder.cpp:75-77,288-290)
 *   nfcgpu_stream_open                 one `lab::NfcDecoder` instance == one stream
 *                                      (lib-lab/lab-radio/src/main/include/lab/nfc/NfcDecoder.h:33-122)
 *   nfcgpu_stream_configure            NfcDecoder::setEnableNfcA/B/F/V, setPowerLevelThreshold,
 *                                      setModulationThresholdNfcX, setCorrelationThresholdNfcX, setSampleRate,
 *                                      setStreamTime (NfcDecoder.cpp:96-286), as driven by
 *                                      RadioDecoderTask::configDecoder (lib-lab/lab-tasks/src/main/cpp/tasks/RadioDecoderTask.cpp:207-366)
 *   nfcgpu_stream_reset                NfcDecoder::initialize() (NfcDecoder.cpp:295-360)
 *   nfcgpu_submit                      NfcDecoder::nextFrames(hw::SignalBuffer) for a valid buffer
 *                                      (NfcDecoder.cpp:374-447); stride 1 = SIGNAL_TYPE_RADIO_SAMPLES magnitude,
 *                                      stride 2 = SIGNAL_TYPE_RADIO_IQ with the IQ->magnitude step of
 *                                      RadioDeviceTask::processQueue (lab-tasks/.../RadioDeviceTask.cpp:547-656) fused in
 *   nfcgpu_submit_batch / _uniform     the same call for many independent streams at once (the reference would run one
 *                                      NfcDecoder per stream on one thread each); inputs may already be resident in HBM
 *   nfcgpu_submit_fmt / _batch_fmt /   the same calls for samples in the format capture files hold them in: 16-bit PCM, as
 *   _uniform_fmt, nfcgpu_magnitude_fmt SignalStorageTask::writeRadio records and readRadio replays. The kernels convert while they
 *                                      load, value = (float)v / 32768.0f: the widening hw::RecordDevice::readScaledSamples<short>
 *                                      does on the host (lib-hw/hw-radio .../RecordDevice.cpp:247-248, 281-311) and the fp32 copy
 *                                      of the capture it makes are skipped
 *   nfcgpu_spectrum_fmt,               the display consumers of the same buffers - FourierProcessTask (lab-tasks/.../FourierProcessTask.cpp)
 *   nfcgpu_resample_radio_fmt          and SignalResamplingTask (SignalResamplingTask.cpp:168-226) - reading that format in place too
 *   nfcgpu_flush                       NfcDecoder::nextFrames(invalid buffer) -> one carrier-state frame (NfcDecoder.cpp:449-463)
 *   nfcgpu_poll                        the returned std::list<lab::RawFrame> (lab-data/src/main/cpp/RawFrame.cpp:26-98)
 *   nfcgpu_stream_close                ~NfcDecoder
 *
 * Conventions: every function returns 0 on success or a negative NFCGPU_E* code; no exceptions cross the ABI;
 * outputs are caller-allocated; input buffers are never retained past the call that received them unless they are
 * device-resident (then they must stay valid until nfcgpu_sync / nfcgpu_poll returns). One thread per context.
 * There is no CPU fallback: without a usable gfx950 device nfcgpu_init fails with NFCGPU_ENODEV.
 */
#ifndef NFCGPU_H
#define NFCGPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NFCGPU_OK 0
#define NFCGPU_EINVAL (-1)    /* bad argument */
#define NFCGPU_ENODEV (-2)    /* no usable HIP device / kernel image */
#define NFCGPU_ENOMEM (-3)    /* allocation failed, or more than 256 distinct decoder configurations in use at once */
#define NFCGPU_ESTREAM (-4)   /* unknown or closed stream id */
#define NFCGPU_ERATE (-5)     /* sample rate not decodable (history depth) */
#define NFCGPU_EOVERFLOW (-6) /* frame sink overflowed, frames were dropped */
#define NFCGPU_EHIP (-7)      /* HIP runtime error, see nfcgpu_last_error */
#define NFCGPU_EFULL (-8)     /* no free stream slot */
#define NFCGPU_EIO (-9)       /* a file could not be opened or written (nfcgpu_trace_write*) */

#define NFCGPU_TECH_A 0x1u
#define NFCGPU_TECH_B 0x2u
#define NFCGPU_TECH_F 0x4u
#define NFCGPU_TECH_V 0x8u

#define NFCGPU_LOC_HOST 0u
#define NFCGPU_LOC_DEVICE 1u

/* sample formats of the decoder's input (the _fmt entry points; one format per call, as one stride per call) */
#define NFCGPU_FMT_F32 0u /* float, what every entry point without _fmt takes */
#define NFCGPU_FMT_I16 1u /* little-endian int16 PCM, value = (float)v / 32768.0f (RecordDevice.cpp:247-248, 297-300) */

typedef struct nfcgpu_ctx nfcgpu_ctx;

/* decoder configuration of one stream; defaults (nfcgpu_default_params) are the reference's
 * (NfcTech.h:347, NfcA.cpp:94-100, NfcB.cpp:103-109, NfcF.cpp:88-94, NfcV.cpp:101-107) */
typedef struct nfcgpu_params
{
   uint32_t sample_rate;          /* Hz; 0 = take it from the first submitted buffer */
   uint32_t tech_mask;            /* NFCGPU_TECH_* */
   int64_t stream_time;           /* reference time added to frame dateTime (NfcDecoder::setStreamTime) */
   float power_level_threshold;
   float corr_threshold[4];       /* A B F V */
   float min_modulation_depth[4]; /* A B F V */
   float max_modulation_depth[4]; /* A B F V */
} nfcgpu_params;

/* one decoded frame == the compared fields of lab::RawFrame plus payload (RawFrame.cpp:82-98) */
typedef struct nfcgpu_frame
{
   uint32_t stream_id;
   uint32_t tech_type;   /* lab::FrameTech  */
   uint32_t frame_type;  /* lab::FrameType  */
   uint32_t frame_flags; /* lab::FrameFlags */
   uint32_t frame_phase; /* lab::FramePhase */
   uint32_t frame_rate;
   uint32_t length;
   uint32_t reserved;
   uint64_t sample_start;
   uint64_t sample_end;
   uint64_t sample_rate;
   uint8_t data[512];
} nfcgpu_frame;

typedef struct nfcgpu_options
{
   uint32_t max_streams;     /* stream slots reserved in HBM (rounded up to 64); default 1024 */
   uint32_t reserved;
   uint64_t frame_sink_bytes; /* device frame sink per sync interval; default 64 MiB */
} nfcgpu_options;

/* many streams, one call. data[i] points to n_samples[i]*stride floats of stream stream_ids[i] (nfcgpu_submit_batch_fmt: values
 * of the call's format) */
typedef struct nfcgpu_batch
{
   uint32_t n_streams;
   uint32_t stride;      /* 1 magnitude, 2 interleaved IQ */
   uint32_t location;    /* NFCGPU_LOC_* of every data[i] */
   uint32_t sample_rate; /* Hz */
   const uint32_t *stream_ids;
   const void *const *data;
   const uint32_t *n_samples;
} nfcgpu_batch;

/* accumulated since nfcgpu_stats_reset; kernel_ms is HIP-event time of the demodulation kernel on the context's stream */
typedef struct nfcgpu_stats
{
   uint64_t launches;
   uint64_t samples;
   uint64_t frames;
   uint64_t dropped_frames;
   double kernel_ms;
   /* time-parallel path: scan kernel time and samples (profiling on), windowed decode kernel time,
    * windows decoded (lanes, repeats included), decode passes, streams of submissions that took it / fell back */
   double scan_ms;
   double window_ms;
   uint64_t scan_samples;
   uint64_t windows;
   uint64_t window_passes;
   uint64_t windowed_streams;
   uint64_t fallback_streams;
   uint64_t scan_repairs; /* scan chunks walked a second time because their warm-up had not reached the true state */
   /* round 3 (read through nfcgpu_stats_get_sized by callers built against this header; nfcgpu_stats_get fills the
    * fields above only): the wave decoder's kernel - HIP-event time of all its launches and their number - and the walk
    * that writes the front-end planes for it */
   double wave_ms;
   uint64_t wave_launches;
   double planes_ms;
   /* round 4: the time the wave decoder's kernel was running at all since nfcgpu_stats_reset - the union of its launch
    * intervals (the carry lanes of a pass run on a second HIP stream beside the speculative lanes, so wave_ms, the sum of
    * the launch durations, counts the overlap twice). Profiling on; measured from the reset on. */
   double wave_busy_ms;
   /* pipelined submissions (read through nfcgpu_stats_get_sized): submissions whose front - scan, seam rounds, planes - ran under
    * the pending tail of the submission before, and streams whose front was walked again because the state the finish left in
    * their slot was not the one that front had started from (exact or not taken) */
   uint64_t pipelined_submissions;
   uint64_t pipeline_refronts;
   /* ... and streams of pipelined submissions that ended on an edge time zeroed by a carrier frame where the shadow held the
    * tracker's time: the one expected difference, put right in the front's records without a walk (not counted above) */
   uint64_t pipeline_zeroed_edges;
} nfcgpu_stats;

#define NFCGPU_STATS_SIZE_V2 104u /* bytes of nfcgpu_stats up to and including scan_repairs: what nfcgpu_stats_get writes */

void nfcgpu_default_params(nfcgpu_params *params);

int nfcgpu_init(int device, const nfcgpu_options *options, nfcgpu_ctx **ctx);
int nfcgpu_shutdown(nfcgpu_ctx *ctx);

int nfcgpu_stream_open(nfcgpu_ctx *ctx, const nfcgpu_params *params, uint32_t *stream_id);
int nfcgpu_stream_open_many(nfcgpu_ctx *ctx, const nfcgpu_params *params, uint32_t count, uint32_t *first_stream_id);
/* The setters of lab::NfcDecoder (NfcDecoder.cpp:96-286). The enable mask and the per-technology thresholds take effect
 * with the next sample; the power level moves the detectors' gate at once and the carrier thresholds at the next
 * initialisation (NfcDecoder.cpp:327-329); sample_rate is only stored (0 leaves it as it is), exactly like
 * setSampleRate(): nothing is derived from it until the stream (re)initialises. */
int nfcgpu_stream_configure(nfcgpu_ctx *ctx, uint32_t stream_id, const nfcgpu_params *params);
/* initialize() (NfcDecoder.cpp:295-360): clock, detectors, protocol state and everything derived from the sample rate and
 * the power level stored at this moment start over; envelope, filter and carrier state carry on. Applied when the next
 * buffer arrives; an nfcgpu_flush() in between already sees the reset clock. */
int nfcgpu_stream_reset(nfcgpu_ctx *ctx, uint32_t stream_id);
int nfcgpu_stream_close(nfcgpu_ctx *ctx, uint32_t stream_id);

/* nextFrames(valid buffer) (NfcDecoder.cpp:374-447) without the frame collection (nfcgpu_poll). A buffer whose sample rate
 * differs from the stored one stores it and re-initialises the stream first, also when it is empty (n_samples 0); a
 * buffer at the stored rate does not, whatever the stored rate was derived-from last (see nfcgpu_stream_configure). */
/* Submissions are asynchronous: the calls return once the work is enqueued on the context's HIP stream. Host memory
 * (NFCGPU_LOC_HOST, nfcgpu_submit) has been copied into a pinned staging buffer by then and is never retained; device
 * memory (NFCGPU_LOC_DEVICE) is read in place and must stay as it is until the next nfcgpu_sync / nfcgpu_poll /
 * nfcgpu_flush / nfcgpu_pending of the context. That holds for every submission: a long grid-aligned one that takes the
 * time-parallel path through nfcgpu_submit_uniform returns once its first decode pass is queued; its last passes and the finish
 * stay pending on the context, and the next such submission of the same streams walks its front end beside them. Every other
 * call on the context completes what is pending before it does anything else, and returns an error met there. */
int nfcgpu_submit(nfcgpu_ctx *ctx, uint32_t stream_id, const float *data, uint32_t n_samples, uint32_t stride, uint32_t sample_rate);
int nfcgpu_submit_batch(nfcgpu_ctx *ctx, const nfcgpu_batch *batch);
/* streams first..first+count-1; stream i reads n_samples*stride floats at base + i*pitch_bytes */
int nfcgpu_submit_uniform(nfcgpu_ctx *ctx, uint32_t first_stream_id, uint32_t count, const void *base, uint64_t pitch_bytes,
                          uint32_t n_samples, uint32_t stride, uint32_t location, uint32_t sample_rate);

/* The same calls with a sample format (NFCGPU_FMT_*). `stride` keeps its meaning (1 magnitude, 2 interleaved IQ); a sample is
 * stride * 4 bytes of NFCGPU_FMT_F32 or stride * 2 bytes of NFCGPU_FMT_I16, and data pointers, base and pitch_bytes must be
 * multiples of that (2 bytes for int16 magnitude, 4 for int16 IQ; NFCGPU_EINVAL otherwise, as for an unknown format). With
 * NFCGPU_FMT_F32 they are the calls above, to the error codes and texts. The kernels read int16 where it lies - host input
 * is staged as int16, n * stride * 2 bytes per row, device input is read in place - and convert on load; no fp32 copy of a
 * submission is made. The conversion is exact (a power-of-two scale of a 16-bit integer; IQ components are converted and
 * then go through the same magnitude formula), so any sequence of calls with int16 buffers gives exactly the frames, in
 * every field and in the same order, that it gives with float buffers holding (float)v / 32768.0f - and takes the
 * time-parallel path exactly when those would. A stream may receive floats in one call and int16 in the next: stream
 * state does not know the format. */
int nfcgpu_submit_fmt(nfcgpu_ctx *ctx, uint32_t stream_id, const void *data, uint32_t n_samples, uint32_t stride, uint32_t sample_rate,
                      uint32_t format);
int nfcgpu_submit_batch_fmt(nfcgpu_ctx *ctx, const nfcgpu_batch *batch, uint32_t format);
int nfcgpu_submit_uniform_fmt(nfcgpu_ctx *ctx, uint32_t first_stream_id, uint32_t count, const void *base, uint64_t pitch_bytes,
                              uint32_t n_samples, uint32_t stride, uint32_t location, uint32_t sample_rate, uint32_t format);

/* Magnitude of interleaved float IQ, out[i] = sqrtf(I*I + Q*Q) with the reference's roundings (products and sum
 * rounded separately, correctly rounded root): the conversion RadioDeviceTask applies before publishing a
 * SIGNAL_TYPE_RADIO_SAMPLES buffer (RadioDeviceTask.cpp:547-656, scalar form 626-642). The decoder entry points do
 * this on the fly for stride-2 input; this call exposes the same device function for hosts that also want the
 * magnitudes (storage, display) and for bit-exact testing. `location` applies to both pointers; the call returns
 * when `out` is complete. */
int nfcgpu_magnitude(nfcgpu_ctx *ctx, const float *iq, uint64_t n_samples, float *out, uint32_t location);
/* the same for IQ in `format`: int16 components (4-byte aligned pairs) are converted, (float)v / 32768.0f, then the same formula */
int nfcgpu_magnitude_fmt(nfcgpu_ctx *ctx, const void *iq, uint64_t n_samples, float *out, uint32_t location, uint32_t format);

/* Adaptive resampling of magnitude buffers for display, the radio branch of the reference's SignalResamplingTask
 * (SignalResamplingTask.cpp:168-226: `processRadioSignal`, the other per-sample consumer of "radio.signal.raw"): every
 * buffer of n_samples floats is reduced to (value, sample offset) control points wherever the sample departs from its
 * 51-sample centred mean by more than 0.005, or every 255 samples; each buffer is independent (the running mean
 * restarts with it), the output of buffer b is written as float pairs at out + b * out_pitch_bytes and its pair count
 * to counts[b] — the contents of the SIGNAL_TYPE_RADIO_SIGNAL buffer the reference publishes on "adaptive.signal".
 * capacity_pairs bounds what is written per buffer (the worst case is n_samples + n_samples / 255 + 2 pairs); a buffer
 * that needs more keeps counting and the call returns NFCGPU_EOVERFLOW. n_samples >= 25. `out` and out_pitch_bytes are 8-byte aligned. `location` applies to `in`,
 * `out` and `counts` alike. */
int nfcgpu_resample_radio(nfcgpu_ctx *ctx, const float *in, uint64_t in_pitch_bytes, uint32_t n_buffers, uint32_t n_samples,
                          float *out, uint64_t out_pitch_bytes, uint32_t capacity_pairs, uint32_t *counts, uint32_t location);
/* The same for buffers of samples as the decoder takes them: `stride` 1 magnitude or 2 interleaved IQ, `format` NFCGPU_FMT_*, so
 * that a capture that is decoded in place is drawn in place. The resampled value is the magnitude the decoder's loader forms of
 * a sample - (float)v / 32768.0f of int16 (RecordDevice.cpp:247-248, 297-300), and for IQ the formula of nfcgpu_magnitude on the
 * converted pair (RadioDeviceTask.cpp:626-642), which is what RadioDeviceTask publishes on "radio.signal.raw" for
 * SignalResamplingTask.cpp:168-226 to read - formed while the kernel loads; the control points of a buffer are bit for bit those
 * nfcgpu_resample_radio gives for a float buffer holding these magnitudes, and no such buffer is made: host input is staged in
 * its own format, device input is read in place. `in` and in_pitch_bytes are multiples of a sample (stride * 4 bytes of
 * NFCGPU_FMT_F32, stride * 2 of NFCGPU_FMT_I16: an int16 magnitude row may start on any 2-byte boundary), in_pitch_bytes at
 * least n_samples of them; NFCGPU_EINVAL otherwise, as for a stride or format that is not one of these. out, counts,
 * capacity_pairs, NFCGPU_EOVERFLOW and n_samples >= 25 are as above. With stride 1 and NFCGPU_FMT_F32 it is the call above, to
 * the error codes and texts (a misaligned `in` is refused here). */
int nfcgpu_resample_radio_fmt(nfcgpu_ctx *ctx, const void *in, uint64_t in_pitch_bytes, uint32_t n_buffers, uint32_t n_samples,
                              uint32_t stride, uint32_t format, float *out, uint64_t out_pitch_bytes,
                              uint32_t capacity_pairs, uint32_t *counts, uint32_t location);

/* Spectrum of interleaved float IQ for display: what the reference's FourierProcessTask, the consumer of "radio.signal.iq",
 * publishes on "signal.fft" (lab-tasks/src/main/cpp/tasks/FourierProcessTask.cpp, the SSE2 branches that
 * lab-tasks/CMakeLists.txt:18 builds), for every frame of every buffer instead of one buffer every 10 ms:
 *   - length 1024, window "Hamming", bandwidth 625 000 Hz (:45-49, :86); decimation D = int(sample rate / bandwidth) (:239),
 *     16 at 10 MS/s; a buffer with fewer than L * D elements gives nothing (:242);
 *   - window tables (:121-143) under the reference's names, which are not what they compute: "Hamming" is
 *     float(pow(sin(float(M_PI * n / L)), 2)), a periodic Hann; "Hann" is float(0.5 * (1.0 - cos(2.0 * M_PI * n / (L - 1)))),
 *     the symmetric one; anything else is 1;
 *   - input (:250-262): eight floats out of every 8 D, times the window in fp32: FFT input m is the source pair
 *     4 * D * (m >> 2) + (m & 3), four consecutive pairs out of every 4 D, not every D-th pair;
 *   - forward complex FFT, unnormalised (:276); sqrtf(re * re + im * im), products and sum rounded separately (:279-341);
 *   - L floats per frame with the halves swapped: bins L/2 ... L-1 (negative frequencies) first, then 0 ... L/2-1 (:344-348).
 * Window product and magnitude are the reference's operations to the bit; the butterflies are this library's own (the
 * reference's are mufft's), so values agree with the reference's to the rounding error of a float FFT, not bit for bit. */
#define NFCGPU_WINDOW_NONE 0
#define NFCGPU_WINDOW_HAMMING 1
#define NFCGPU_WINDOW_HANN 2

typedef struct nfcgpu_spectrum_params {
   uint32_t length;      /* FFT length L, a power of two, 256 ... 4096; the reference's is 1024 */
   uint32_t window;      /* NFCGPU_WINDOW_NONE 0, NFCGPU_WINDOW_HAMMING 1 (the reference's default), NFCGPU_WINDOW_HANN 2:
                            the reference's tables under the reference's names (see above for what they compute) */
   uint32_t decimation;  /* D >= 1; 0 = derive it as the reference does, sample_rate / 625000 (at least 1) */
   uint32_t hop;         /* IQ pairs between the starts of successive frames of one buffer; 0 = one frame at pair 0,
                            which is what FourierProcessTask publishes for that buffer */
   uint32_t sample_rate; /* used only when decimation == 0 */
   uint32_t reserved[3]; /* zero */
} nfcgpu_spectrum_params;

void nfcgpu_spectrum_default_params(nfcgpu_spectrum_params *p);   /* 1024, HAMMING, 0, 0, 10000000 */

/* frames a buffer of n_pairs IQ pairs gives: 0 if n_pairs < L*D (the reference's guard, FourierProcessTask.cpp:242), else 1
 * for hop == 0, else (n_pairs - L*D) / hop + 1. 0 also for parameters nfcgpu_spectrum refuses. */
uint32_t nfcgpu_spectrum_frames(const nfcgpu_spectrum_params *p, uint32_t n_pairs);

/* Buffer b is n_pairs interleaved IQ pairs at iq + b * in_pitch_bytes (8-byte aligned, in_pitch_bytes a multiple of 8); its
 * frames f = 0 ... frames-1 start at pair f * hop and are written as L floats each, in the reference's order, at
 * out + b * out_pitch_bytes + f * L * 4 (out_pitch_bytes a multiple of 16 and at least frames * L * 4;
 * bytes of a pitch beyond the frames are left alone). One launch transforms all n_buffers * frames frames
 * (FourierProcessTask::process(), :236-355, is one frame). `location` applies to `iq` and `out`; the call returns when `out`
 * is complete. Zero frames is success and writes nothing. */
int nfcgpu_spectrum(nfcgpu_ctx *ctx, const float *iq, uint64_t in_pitch_bytes, uint32_t n_buffers, uint32_t n_pairs,
                    const nfcgpu_spectrum_params *params, float *out, uint64_t out_pitch_bytes, uint32_t location);
/* The same for IQ in `format` (NFCGPU_FMT_*). With NFCGPU_FMT_F32 it is the call above, to the error codes and texts. With
 * NFCGPU_FMT_I16 a pair is two little-endian int16, I then Q, as a two-channel capture file holds them: iq and in_pitch_bytes are
 * multiples of 4 (not 8), so a frame, which starts at pair f * hop, starts at any 4-byte boundary. Both components are converted as
 * they are loaded, (float)v / 32768.0f (RecordDevice.cpp:247-248, 297-300; exact), and then take the window product (:250-262),
 * the butterflies, the magnitude (:279-341) and the swap of halves (:344-348) of the float call: the floats written are bit for bit
 * those of nfcgpu_spectrum on a float buffer holding the converted values, and no such buffer is made - host input is staged as
 * int16, n_pairs * 4 bytes per row, device input is read in place. Frame counts, the n_pairs < L * D guard (:242), `out` and its
 * pitch, and zero frames being success are those of the float call, and so is what is not checked: in_pitch_bytes may be smaller
 * than a row in either format (input rows may overlap; they are only read). NFCGPU_EINVAL also for an unknown format. */
int nfcgpu_spectrum_fmt(nfcgpu_ctx *ctx, const void *iq, uint64_t in_pitch_bytes, uint32_t n_buffers, uint32_t n_pairs,
                        const nfcgpu_spectrum_params *params, float *out, uint64_t out_pitch_bytes, uint32_t location,
                        uint32_t format);

/* Recording: float samples to the 16-bit PCM of a capture file, with the receiver's levels, in one pass over the input - the
 * per-sample loop of SignalStorageTask::writeRadio (SignalStorageTask.cpp:493-523, hw::RecordDevice::writeScaledSamples<short>,
 * RecordDevice.cpp:313-348) and the level part of the magnitude loop of RadioDeviceTask::processQueue
 * (RadioDeviceTask.cpp:547-680).
 *
 * Buffer b is n_samples * stride floats at in + b * in_pitch_bytes (`in` and in_pitch_bytes multiples of 4 * stride) and is
 * written as n_samples * channels int16 at out + b * out_pitch_bytes (`out` and out_pitch_bytes multiples of 2 * channels and
 * no more: a mono row may start on any 2-byte boundary; out_pitch_bytes at least the row; bytes of a pitch beyond the row are
 * left alone). channels is 2 for stride 2 with NFCGPU_RECORD_SAME, else 1. NFCGPU_RECORD_MAGNITUDE (stride 2 only) records
 * the magnitude the decoder's loader forms of an I/Q sample (nfcgpu_magnitude), so decoding the recording sees the
 * magnitudes the decoder would have computed of the floats, quantised.
 *
 * A value v becomes t = v * 32768.0f (one fp32 product), q = t rounded toward zero; -32768 <= q <= 32767 is written as it is:
 * for finite input in range that is the reference's static_cast<short>(v * 32768.0f), and k / 32768.0f gives k for every int16
 * k (recording is a left inverse of NFCGPU_FMT_I16 input). One departure from the reference: outside that range its cast is
 * undefined (on x86 it wraps: 1.0 is written as -32768); here values beyond the range and infinities saturate to 32767 or
 * -32768 and NaN is written as 0, and every such value counts in `clipped`. Magnitudes of I/Q do exceed 1.0.
 *
 * levels (may be NULL: the reductions are skipped), one record per buffer, over the magnitudes m of the buffer (stride 2, both
 * modes; stride 1: m is the input itself) - what RadioDeviceTask::processQueue derives per buffer:
 *   power    sum(I*I + Q*Q) / n_samples (stride 1: sum(v*v) / n_samples), :623 / :646
 *   average  the AGC average (:617-620 / :639, compared with 0.05 and 0.25 at :666-679): a = 0; for k = 0 ... ceil(n / 4) - 1:
 *            a = a * (1 - 0.001f) + m[4 k] * 0.001f - the reference's recurrence over every fourth magnitude, restarted per
 *            buffer; evaluated in parallel, within 2048 * 2^-24 relative of the exact value for non-negative m
 *   peak     the largest m (stride 1: the largest value), NaNs ignored; 0 when there is none
 *   clipped  PCM values written that were saturated or came from a NaN
 * power is summed pairwise (no value passes through more than 60 additions). Results do not depend on the run, on the other
 * buffers of the call or on where the rows lie. `location` applies to `in`, `out` and `levels`; the call returns when they are
 * complete. n_samples == 0 or n_buffers == 0 is success and writes no PCM (levels of n_samples == 0 are all zero). */
#define NFCGPU_RECORD_SAME 0u       /* stride 1 -> mono PCM; stride 2 -> two-channel I/Q PCM, interleaved */
#define NFCGPU_RECORD_MAGNITUDE 1u  /* stride 2 only: magnitude (nfc_iq_magnitude) -> mono PCM */

typedef struct nfcgpu_record_levels {   /* one per buffer, 16 bytes */
   float power;
   float average;
   float peak;
   uint32_t clipped;
} nfcgpu_record_levels;

int nfcgpu_record(nfcgpu_ctx *ctx, const float *in, uint64_t in_pitch_bytes, uint32_t n_buffers, uint32_t n_samples,
                  uint32_t stride, uint32_t mode, int16_t *out, uint64_t out_pitch_bytes,
                  nfcgpu_record_levels *levels /* may be NULL */, uint32_t location);

/* The signal debug tap: what the decoder's front end makes of every sample, as planes of floats - the values
 * NfcDecoderStatus::nextSample (NfcTech.cpp:28-105) hands to NfcSignalDebug with setEnableDebug(true) (:94-102, channels 0-3 of
 * radio-debug-*.wav: samplingValue, filteredValue, meanDeviation, signalAverage), and the two the detectors gate on, the envelope
 * (:39-53, against the power threshold) and the modulation depth (:74, against min / max_modulation_depth).
 *
 * Buffer b is n_samples samples of `stride` (1 magnitude, 2 interleaved I/Q) and `format` (NFCGPU_FMT_*) at in + b * in_pitch_bytes;
 * `in` and in_pitch_bytes are multiples of a sample (stride * 4 bytes of NFCGPU_FMT_F32, stride * 2 of NFCGPU_FMT_I16), as for
 * the _fmt submit calls, and samples are loaded exactly as those load them. The k-th channel selected in params->channels, in bit
 * order, is written as n_samples floats at out + b * out_pitch_bytes + k * plane_pitch_bytes (planar; `out` 4-byte aligned,
 * both pitches multiples of 16, plane_pitch_bytes >= 4 * n_samples, out_pitch_bytes at least the planes of a buffer when there
 * is more than one buffer; bytes beyond a plane's n_samples floats are left alone). state_in / state_out are n_buffers
 * records (4-byte aligned). `location` applies to in, out, state_in and state_out; `report` is host memory. The call returns
 * when `out` is complete. n_samples == 0 or n_buffers == 0 is success and writes no planes; state_out is then state_in.
 *
 * Every float written is the value the device step machine produces when it is given the buffer sample by sample from
 * state_in - per sample ++clock, ++pulse_filter, the front end, the depth - bit for bit (a NaN where that walk gives a NaN, such
 * as the depth of a first sample of 0), and state_out is that walk's state behind the last sample. The buffers are cut into
 * chunks that are walked side by side, each from a guess some samples ahead of it, and every chunk whose walk did not start in
 * the very state the chunk before it ended in is walked again from there, round after round, until none is left: results
 * do not depend on chunk_samples, warm_samples, n_buffers, where the rows lie, or the run. report: chunks in all, rounds of
 * second walks, chunks walked twice.
 *
 * NFCGPU_EINVAL: a NULL or misaligned pointer, channels 0 or with unknown bits, a stride, format, location, pitch or chunk_samples
 * that is not as above, reserved fields that are not zero, sample_rate 0, more than 2^32 - 1 chunks. NFCGPU_ERATE: a sample rate
 * the decoder refuses.
 *
 * Alignment with the decoder. nfcgpu_stream_tap_state completes what is pending on the context and gives the front-end state the
 * stream's next buffer at its stored rate will start from: that of a stream just opened before its first buffer, after
 * nfcgpu_stream_reset the restarted clock with pulse filter, envelope, filter, deviation and average carried on. Tapping a
 * buffer from that state and then submitting the same buffer gives planes whose index i is the sample the frames' sample_start /
 * sample_end count: sample i of the buffer has the clock state.clock + 1 + i (32-bit), the number a frame carries. */
#define NFCGPU_TAP_VALUE     0x01u /* samplingValue: the sample as the decoder takes it (stride 2: nfc_iq_magnitude of the pair) */
#define NFCGPU_TAP_FILTERED  0x02u /* filteredValue, NfcTech.cpp:55-62 */
#define NFCGPU_TAP_DEVIATION 0x04u /* meanDeviation, :65 */
#define NFCGPU_TAP_AVERAGE   0x08u /* signalAverage, :68 */
#define NFCGPU_TAP_ENVELOPE  0x10u /* signalEnvelope after this sample's update, :39-53 */
#define NFCGPU_TAP_DEPTH     0x20u /* modulateDepth, :74 */

typedef struct nfcgpu_tap_state {   /* 32 bytes: what the front end carries from one sample to the next */
   uint32_t clock, pulse_filter;
   float envelope, filter_n1, deviation, average;
   uint32_t reserved[2];            /* zero */
} nfcgpu_tap_state;

typedef struct nfcgpu_tap_params {
   uint32_t sample_rate;   /* Hz: the weights and the elementary time unit are the decoder's for this rate (NfcDecoder.cpp:295-360) */
   uint32_t channels;      /* NFCGPU_TAP_* mask, not 0 */
   uint32_t chunk_samples; /* 0 = the library's choice; else a multiple of 64: samples one walker takes */
   uint32_t warm_samples;  /* used with chunk_samples != 0: samples a walker runs before its chunk from a guessed state (0 allowed) */
   uint32_t reserved[4];   /* zero */
} nfcgpu_tap_params;

typedef struct nfcgpu_tap_report { uint32_t chunks, rounds, rewalked_chunks, reserved; } nfcgpu_tap_report;

void nfcgpu_tap_state_init(nfcgpu_tap_state *s);   /* a stream just opened: clock 0xFFFFFFFF, the rest 0 */

int nfcgpu_signal_tap(nfcgpu_ctx *ctx, const void *in, uint64_t in_pitch_bytes, uint32_t n_buffers, uint32_t n_samples,
                      uint32_t stride, uint32_t format, const nfcgpu_tap_params *params,
                      const nfcgpu_tap_state *state_in /* n_buffers, NULL = all freshly opened */,
                      float *out, uint64_t out_pitch_bytes, uint64_t plane_pitch_bytes,
                      nfcgpu_tap_state *state_out /* n_buffers, may be NULL */,
                      nfcgpu_tap_report *report /* host memory, may be NULL */, uint32_t location);

int nfcgpu_stream_tap_state(nfcgpu_ctx *ctx, uint32_t stream_id, nfcgpu_tap_state *state /* host */);

/* The tap reduced over sample ranges: for every range and every channel selected in tap->channels min, max, where they lie, the
 * mean and the count of the values nfcgpu_signal_tap would have written for those samples - a few numbers per frame (the depth
 * a frame reached, at what envelope) or per pixel column of an overview of a long capture - without a plane ever reaching the
 * caller. in, in_pitch_bytes, n_buffers, n_samples, stride, format, tap, state_in, state_out and report are those of
 * nfcgpu_signal_tap and are refused for the same reasons with the same codes; report is the sum over the slabs (below).
 * `location` applies to in, state_in, state_out, ranges and out; `out` is 4-byte aligned.
 *
 * Ranges. Range r is the samples first ... first + count - 1 of buffer `buffer`; ranges may overlap and come in any order. With
 * ranges == NULL (n_ranges must be 0, reduce->bin_samples > 0) every buffer is cut into bins = ceil(n_samples / bin_samples) bins
 * of bin_samples samples (the last one may be short) and range r is bin r % bins of buffer r / bins. With K channels selected the
 * record of range r and the k-th selected channel (bit order) is out[r * K + k].
 *
 * A record. Let p be the plane nfcgpu_signal_tap writes for the buffer and channel, and S the samples of the range where p is no
 * NaN (the depth of a first sample of 0 is one). valid = |S|. argmin is the smallest index i in S (a sample index of the buffer)
 * such that no j in S has p[j] < p[i], and min is p[argmin] with its bits: a -0.0 stays -0.0, infinities are ordinary values;
 * max and argmax likewise with >. mean is the sum of p over S, taken in double, divided by valid and rounded once to float. An
 * empty S (count == 0, or nothing but NaNs) gives min = max = mean = the quiet NaN 0x7FC00000, argmin = argmax = 0xFFFFFFFF,
 * valid = 0. reserved is written as zero. min, max, argmin, argmax and valid do not depend on how the tap or the reduction cut
 * the buffers, on scratch_bytes, the other ranges, the other buffers or the run. mean is the same bits from run to run and for
 * any scratch_bytes: the order of its additions depends only on a sample's offset within its range (segments of 16 384 samples,
 * within one the quads of four a lane of a wave takes, a butterfly over the wave, the segments in order); it is within
 * 2^-24 |m| + (ceil(count / 64) + 7) 2^-53 mean(|p|) of the exact mean m.
 *
 * Memory. The planes exist only in scratch the context owns (freed by nfcgpu_shutdown): the tap runs over a slab of whole buffers,
 * as many as fit into scratch_bytes of planes (4 * n_samples rounded up to 256, times K, per buffer) and at least one, the slab is
 * reduced, the next follows. Every slab pays the tap's rounds of second walks anew, so scratch_bytes == 0 takes all the planes at
 * once where they fit into three quarters of the device memory that is free, and as many buffers as do otherwise. Host input is
 * uploaded once. Beside the planes the call holds 32 bytes
 * per segment of 16 384 samples (or part of one) of every range of a slab and channel, and 8 per segment of every range given.
 *
 * NFCGPU_EINVAL, beyond the tap's: reduce NULL or with non-zero reserved fields; ranges == NULL with bin_samples == 0 or
 * n_ranges != 0; out NULL or misaligned; more than 2^32 - 1 records; a range with buffer >= n_buffers, first + count > n_samples
 * or reserved != 0. Ranges in host memory are checked before anything runs: the call writes nothing. Ranges in device memory are
 * checked by the kernels, which read nothing through such a range: it gets the empty record, every other record and state_out
 * are complete, and the call returns NFCGPU_EINVAL. n_ranges == 0 with ranges != NULL and n_samples == 0 (every range then has
 * count 0) are success, state_out as the tap leaves it; n_buffers == 0 is success and writes nothing. */
typedef struct nfcgpu_tap_range { uint32_t buffer, first, count, reserved; } nfcgpu_tap_range;

typedef struct nfcgpu_tap_stat {   /* 32 bytes: one channel over one range */
   float min, max, mean;
   uint32_t valid;                 /* samples of the range whose value is not a NaN */
   uint32_t argmin, argmax;        /* sample index in the buffer */
   uint32_t reserved[2];           /* written as zero */
} nfcgpu_tap_stat;

typedef struct nfcgpu_tap_reduce_params {
   uint32_t bin_samples;    /* with ranges == NULL: samples of a bin */
   uint32_t reserved0;      /* zero */
   uint64_t scratch_bytes;  /* bound on the device memory the call uses for planes at a time; 0 = what three quarters of the free device memory hold. At least one buffer is always taken */
   uint32_t reserved[4];    /* zero */
} nfcgpu_tap_reduce_params;

int nfcgpu_signal_tap_reduce(nfcgpu_ctx *ctx, const void *in, uint64_t in_pitch_bytes, uint32_t n_buffers, uint32_t n_samples,
                             uint32_t stride, uint32_t format, const nfcgpu_tap_params *tap, const nfcgpu_tap_reduce_params *reduce,
                             const nfcgpu_tap_state *state_in /* n_buffers, NULL = all freshly opened */,
                             const nfcgpu_tap_range *ranges /* n_ranges, NULL = bins */, uint32_t n_ranges,
                             nfcgpu_tap_stat *out /* records */, nfcgpu_tap_state *state_out /* n_buffers, may be NULL */,
                             nfcgpu_tap_report *report /* host memory, may be NULL */, uint32_t location);

/* The signal of a trace file: the control points nfcgpu_resample_radio[_fmt] leaves in memory, delta-coded into the
 * "radio-<id>.apcm" entries the reference's TraceStorageTask stores beside frame.json (writeRadioEntry,
 * lab-tasks/src/main/cpp/tasks/TraceStorageTask.cpp:881-1003; read back by readRadioEntry :760-879) - what its signal view draws
 * when the trace is opened. nfcgpu_trace_write_signal puts the entries into the archive.
 *
 * Input: the rows exactly as the resampler writes them - buffer b holds counts[b] float pairs (value, offset in buffer) at
 * pairs + b * pairs_pitch_bytes (`pairs` and the pitch 8-byte aligned, the pitch at least capacity_pairs pairs; capacity_pairs
 * bounds a row). buffers_per_entry = G consecutive buffers are one entry: n_buffers is a multiple of G, entry e is the buffers
 * e * G ... e * G + G - 1 and carries the stream id first_stream_id + e. Buffer j of an entry has the stream position
 * first_position + j * buffer_samples (hw::SignalBuffer::offset()). `location` applies to pairs, counts, out and info.
 *
 * What an entry is. sampleStart = (uint32)(sample_rate * range_start), sampleEnd = (uint32)(sample_rate * range_end): the
 * reference's double product and cast (:907-908). range_start == range_end == 0 means every point (sampleEnd = 2^32 - 1): the
 * departure from the reference nfcgpu_trace_write_frames makes for frames, for the same reason. Point by point, in buffer order
 * and then in pair order (:957-970):
 *   offset = position + (uint32)pair.offset (a negative value or a NaN gives 0, the cast saturates above);
 *   sample = the quantiser of nfcgpu_record: static_cast<short>(value * 32768.0f) in range (:969), saturated beyond it, a NaN as
 *            0 - that call's documented departure.
 * A point is kept iff sampleStart <= offset <= sampleEnd. For the monotone offsets the resampler produces this is the reference's
 * `continue` below the range and `break` above it (:972-976). Kept point k becomes three bytes (:979-981): (offset_k -
 * offset_{k-1}) & 0xff, then (sample_k - sample_{k-1}) & 0xffff, low byte first, with offset_{-1} = sampleStart and sample_{-1}
 * = 0 (:953-954). The entry is the 32-byte SampleHdr (:55-60, indices :36-39) - "APCM", version 2, info = {0, 0 (start offset:
 * the reference writes 0), K, stream id, sample_rate, 0} - followed by the K records. Entry e is written at out + e *
 * out_pitch_bytes (`out` and the pitch multiples of 4); bytes of a pitch beyond the entry are left alone. An entry has the same
 * bytes on every run.
 *
 * Results, one per entry: bytes = 32 + 3 K, records = K, wrapped = the records whose offset delta (mod 2^32) was above 255 - the
 * reference loses those silently; it is 0 for resampler output of consecutive buffers with a range inside the data (a point at
 * least every 255 samples). An entry of more than capacity_bytes gets its header, with the number of records that are there in
 * info[2], and the records that fit whole; K is still counted and the call returns NFCGPU_EOVERFLOW, as nfcgpu_resample_radio
 * does. An entry with no kept point is a bare header. n_buffers == 0 is success. nfcgpu_apcm_bound(total_pairs) = 32 + 3 *
 * total_pairs is the size of an entry that keeps total_pairs points.
 *
 * NFCGPU_EINVAL: a NULL context, params or (with n_buffers > 0) pairs, counts, out or info; reserved fields that are not zero; a
 * location that is not one of the two; sample_rate 0; buffers_per_entry 0 or not dividing n_buffers; first_position +
 * buffers_per_entry * buffer_samples (the position of the last buffer's end) not below 2^32; first_stream_id + n_buffers /
 * buffers_per_entry above 2^32; a range that is not 0 <= range_start <= range_end (a NaN is none) or with sample_rate * range_end
 * not below 2^32; pointers or pitches not aligned as above (counts and info: 4 bytes); pairs_pitch_bytes below capacity_pairs
 * pairs; capacity_bytes below 32 or above out_pitch_bytes; buffers_per_entry * capacity_pairs pairs needing 4 GiB or more. A
 * counts[b] above capacity_pairs in host memory is refused before anything runs; in device memory the kernels read capacity_pairs
 * pairs of that buffer and no more, every entry is complete, and the call returns NFCGPU_EINVAL - the rule
 * nfcgpu_signal_tap_reduce has for ranges. */
typedef struct nfcgpu_apcm_params {
   uint32_t sample_rate;        /* Hz: goes into the header and turns the range into samples */
   uint32_t buffers_per_entry;  /* G */
   uint32_t buffer_samples;     /* samples a buffer stands for: the step of the stream position from one buffer to the next */
   uint32_t first_stream_id;    /* entry e carries first_stream_id + e */
   uint32_t first_position;     /* stream position of the first buffer of every entry */
   uint32_t reserved0;          /* zero */
   double range_start, range_end; /* seconds; 0, 0 = every point */
   uint32_t reserved[4];        /* zero */
} nfcgpu_apcm_params;

typedef struct nfcgpu_apcm_info { uint32_t bytes, records, wrapped, reserved; } nfcgpu_apcm_info;   /* one per entry, 16 bytes */

uint64_t nfcgpu_apcm_bound(uint64_t total_pairs);

int nfcgpu_apcm_encode(nfcgpu_ctx *ctx, const float *pairs, uint64_t pairs_pitch_bytes, const uint32_t *counts, uint32_t n_buffers,
                       uint32_t capacity_pairs, const nfcgpu_apcm_params *params, void *out, uint64_t out_pitch_bytes,
                       uint64_t capacity_bytes, nfcgpu_apcm_info *info, uint32_t location);

/* Capture files as hw::RecordDevice writes them (RecordDevice.cpp:493-546, structures :53-100), host only, no context and
 * no device: a 92-byte header - RIFF / WAVE; "fmt " (16: PCM 1, channels, rate, byte rate, block align, 16 bits); "META" (40:
 * "meta", epoch = stream_time, keys[8], the first `channels` taken from `keys`, NULL = zeros); "data" - then the samples,
 * little-endian, interleaved. n_samples counts samples per channel. nfcgpu_wav_append adds samples to a file that starts with
 * exactly this header (the channel count is the header's) and rewrites the RIFF and data sizes. NFCGPU_EIO: the file could not
 * be opened or written. NFCGPU_EINVAL: channels 0 or more than 8, a NULL path, a file that would pass 4 GiB, appending to a
 * file without that header. */
int nfcgpu_wav_write(const char *path, const int16_t *pcm, uint64_t n_samples, uint32_t channels, uint32_t sample_rate,
                     uint32_t stream_time, const int32_t *keys /* NULL = zeros, else `channels` values */);
int nfcgpu_wav_append(const char *path, const int16_t *pcm, uint64_t n_samples);

/* nextFrames(invalid buffer) (NfcDecoder.cpp:449-463): queues one carrier-state frame stamped with the stream's clock */
int nfcgpu_flush(nfcgpu_ctx *ctx, uint32_t stream_id);
/* waits for everything submitted, then moves the frames of the frame sink to the per-stream queues. poll / pending /
 * flush call it; with nothing in flight and nothing to collect none of them touches the device. */
int nfcgpu_sync(nfcgpu_ctx *ctx);
/* Frames wait in a queue per stream until they are polled: nfcgpu_sync moves the frames of every stream there, so a stream
 * that is never polled keeps what it has produced (memory grows with its frames; nfcgpu_stream_close releases it). */
int nfcgpu_poll(nfcgpu_ctx *ctx, uint32_t stream_id, nfcgpu_frame *out, uint32_t capacity, uint32_t *count);
int nfcgpu_pending(nfcgpu_ctx *ctx, uint32_t stream_id, uint32_t *count);

/* Trace files: decoded frames in the format the reference application opens ("open trace") and
 * tools/py_nfclab reads - a gzip-compressed tar archive with one entry frame.json, as TraceStorageTask writes it
 * (lab-tasks/src/main/cpp/tasks/TraceStorageTask.cpp:461-520; read back by :380-449). range_start / range_end in seconds of
 * stream time keep the frames inside the range and shift their times and sample numbers to its start (:461-483, the
 * range of the "write file" command :211-240); 0, 0 = every frame. *written (may be NULL) = frames in the file.
 *   nfcgpu_trace_write_frames  any frames the caller holds (no context, no device);
 *   nfcgpu_trace_write         the frames the device has decoded for a stream and that wait in its queue (nfcgpu_poll
 *                              order; implies nfcgpu_sync); they stay queued. dateTime = the stream's stream_time + timeStart.
 *                              NFCGPU_EINVAL while the sink is held (nfcgpu_sink_hold: nothing is drained into the queues then,
 *                              the file would come out empty).
 * One departure from the reference's writer: with a range it keeps the frames that lie inside it with both ends, as the
 * reference does (timeEnd <= range end); 0, 0 means every frame, where the reference's command always carries a range.
 * "length" is the number of bytes in frameData (at most the 512 a frame record holds). A file that cannot be opened or
 * written is NFCGPU_EIO. */
int nfcgpu_trace_write_frames(const char *path, const nfcgpu_frame *frames, uint32_t count, int64_t stream_time, double range_start, double range_end,
                              uint32_t *written);
int nfcgpu_trace_write(nfcgpu_ctx *ctx, uint32_t stream_id, const char *path, double range_start, double range_end, uint32_t *written);
/* A trace with the signal: frame.json exactly as nfcgpu_trace_write_frames writes it for the same arguments, then one entry
 * "radio-<id>.apcm" per APCM entry (nfcgpu_apcm_encode; host memory), in the order given - the order and the names of
 * writeTraceFile / writeRadioData (TraceStorageTask.cpp:322-364, :1032-1057); <id> is the stream id in the entry's header.
 * entries[i] points to entry_bytes[i] bytes. Host only, no context and no device. With n_entries == 0 the file is byte for byte
 * that of nfcgpu_trace_write_frames. The frames' range is not applied to the entries: they are encoded with theirs.
 * NFCGPU_EINVAL, beyond that call's: entries or entry_bytes NULL with n_entries > 0; an entry that is NULL, shorter than its
 * 32-byte header, without the magic "APCM" or with a version that is not 2; entry_bytes[i] != 32 + 3 * info[2] (what the
 * reference's reader checks, :816-827); two entries with one id; an archive of 4 GiB or more (checked before an entry's records
 * are read). */
int nfcgpu_trace_write_signal(const char *path, const nfcgpu_frame *frames, uint32_t count, int64_t stream_time, double range_start, double range_end,
                              uint32_t *written, const void *const *entries, const uint64_t *entry_bytes, uint32_t n_entries);

/* device-resident view of the frames produced since the last sync: packed records of 32-bit words
 * [stream_id, tech, type, flags, phase, rate, start, end, length, payload...]; used for RCCL frame gathers */
int nfcgpu_sink_device_view(nfcgpu_ctx *ctx, const void **words, const void **cursor_words, uint64_t *capacity_words);
/* use caller-owned device memory as the frame sink (e.g. a torch tensor that RCCL can gather directly):
 * `words` holds capacity_words 32-bit words, `ctl` holds 4 words ([0] cursor in words, [1] dropped frames).
 * Pass words == NULL to return to the context's own sink. Implies a sync + rewind. */
int nfcgpu_sink_attach(nfcgpu_ctx *ctx, void *words, uint64_t capacity_words, void *ctl);
/* when enabled, nfcgpu_sync leaves the sink untouched (no host drain) until nfcgpu_sink_rewind: the caller reads the
 * packed records itself. nfcgpu_poll / nfcgpu_flush then only deal with the per-stream queues filled before; a held sink
 * is meant for hosts that collect frames in bulk (bench.py, RCCL gathers), not to be mixed with polling. */
int nfcgpu_sink_hold(nfcgpu_ctx *ctx, int hold);
int nfcgpu_sink_rewind(nfcgpu_ctx *ctx);

/* ---- multi-GPU: one context (one process) per GPU, streams sharded over the ranks; the only exchange is the gather of
 * the decoded frames, done here in C++ over RCCL so that a host that is not Python (the Qt application,
 * nfc-rx) has it too. The unique id is made on rank 0 and carried to the other ranks by whatever the host uses to start
 * its processes (MPI, sockets, a file, torch.distributed). librccl.so is looked up when the first of these is called. */
#define NFCGPU_UNIQUE_ID_BYTES 128
int nfcgpu_comm_unique_id(void *id128);
int nfcgpu_comm_init(nfcgpu_ctx *ctx, const void *id128, int rank, int n_ranks);
int nfcgpu_comm_destroy(nfcgpu_ctx *ctx);
/* All-gather of every rank's packed frame records (the context's frame sink as it stands: nfcgpu_sink_hold must be on,
 * so that nothing has been drained - NFCGPU_EINVAL otherwise): one ncclAllGather of (word count, receive capacity) per
 * rank, on which every rank takes the same go / no-go decision (NFCGPU_ENOMEM everywhere when some rank's buffer is too
 * small), then the records at their exact sizes (one ncclBroadcast per rank, grouped). `gathered` is a device buffer of
 * capacity_words words; counts_host[r] = words of rank r.
 *   nfcgpu_gather_frames_packed  rank r's records start at the sum of counts_host[0 .. r-1] (needs the sum of the counts);
 *   nfcgpu_gather_frames         the layout of rounds 1-2: rank r's records start at r * *stride_words, *stride_words = the
 *                                largest count (needs n_ranks times that). Round 3 returned the packed layout with a stride
 *                                of 0 under this symbol; a caller built against the older header reads every rank at
 *                                r * stride, so the padded layout is what this symbol keeps.
 * Record format of the sink: [stream, tech, type, flags, phase, rate, start, end, length, payload words]. */
int nfcgpu_gather_frames(nfcgpu_ctx *ctx, void *gathered, uint64_t capacity_words, uint32_t *counts_host, uint64_t *stride_words);
int nfcgpu_gather_frames_packed(nfcgpu_ctx *ctx, void *gathered, uint64_t capacity_words, uint32_t *counts_host);

/* streaming-read bandwidth of this GPU over `bytes` of device memory (16-byte loads per lane, grid sized to the chip):
 * the measured denominator of the HBM roofline, next to the vendor peak. Best of `repeats` passes, GB/s. */
int nfcgpu_read_bandwidth(nfcgpu_ctx *ctx, const void *device_ptr, uint64_t bytes, uint32_t repeats, double *gbps);

int nfcgpu_stats_get(nfcgpu_ctx *ctx, nfcgpu_stats *stats); /* writes NFCGPU_STATS_SIZE_V2 bytes (the struct of rounds 1-2) */
/* writes min(size, sizeof(nfcgpu_stats)) bytes: pass sizeof(nfcgpu_stats) of the header the caller was built with */
int nfcgpu_stats_get_sized(nfcgpu_ctx *ctx, void *stats, uint32_t size);
int nfcgpu_stats_reset(nfcgpu_ctx *ctx);
int nfcgpu_profile(nfcgpu_ctx *ctx, int enable);

void *nfcgpu_hip_stream(nfcgpu_ctx *ctx);
const char *nfcgpu_strerror(int code);
const char *nfcgpu_last_error(nfcgpu_ctx *ctx);
const char *nfcgpu_version(void);

#ifdef __cplusplus
}
#endif

#endif
