"""Trace (.trz) writer for decoded frames: the on-disk format the reference application opens (File > Open) and
`tools/py_nfclab` reads, so that the output of a many-stream GPU run can be inspected with the reference's own tools
(SURVEY.md 8(f) rank 4).

Format, as written by the reference's TraceStorageTask::writeFrameEntry
(src/nfc-lib/lib-lab/lab-tasks/src/main/cpp/tasks/TraceStorageTask.cpp:461-520) and read back by its readFrameEntry
(:380-449): a gzip-compressed tar archive with one entry `frame.json` = {"frames": [ {...}, ... ]}, one object per frame
with sampleStart, sampleEnd, sampleRate, timeStart, timeEnd, techType, frameType, frameRate, frameFlags, framePhase,
dateTime and, for frames with payload, frameData ("26" / "04:00" ... upper-case hex separated by colons) and length.
Times follow the decoder: timeStart = sampleStart / sampleRate, dateTime = streamTime + timeStart
(NfcA.cpp frame construction, NfcDecoder.cpp:449-463).

Frames are the tuples used throughout the tests and bench (nfclab_amd.Frame.as_tuple()):
    (techType, frameType, frameFlags, framePhase, frameRate, sampleStart, sampleEnd, sampleRate, payload bytes)

The signal is stored beside the frames as entries `radio-<id>.apcm` (writeRadioEntry :881-1003, readRadioEntry :760-879): a
32-byte header - "APCM", version 2, six words {flags, start offset, samples, stream id, sample rate, 0} - and three bytes per
control point of the adaptive resampler: the offset's delta (one byte) and the 16-bit sample's delta (little-endian), counted
from (the range's first sample, 0). read_trz_signal sums them up again: offsets come out relative to the start of the range
the writer was given. nfcgpu_apcm_encode (nfclab_amd.NfcGpu.apcm_encode) makes such entries on the GPU.
"""
import io
import json
import struct
import tarfile


def frame_entry(frame, stream_time=0.0):
    tech, ftype, flags, phase, rate, start, end, fs, payload = frame
    time_start = float(start) / float(fs) if fs else 0.0
    time_end = float(end) / float(fs) if fs else 0.0
    entry = {
        "sampleStart": int(start),
        "sampleEnd": int(end),
        "sampleRate": int(fs),
        "timeStart": time_start,
        "timeEnd": time_end,
        "techType": int(tech),
        "frameType": int(ftype),
        "frameRate": int(rate),
        "frameFlags": int(flags),
        "framePhase": int(phase),
        "dateTime": float(stream_time) + time_start,
    }
    if payload:
        entry["frameData"] = ":".join("%02X" % b for b in payload)
        entry["length"] = len(payload)
    return entry


def write_trz(path, frames, stream_time=0.0, signals=None):
    """Write one stream's frames (in stream order) to `path` (must end in .trz). signals: APCM entries (bytes, as
    nfclab_amd.NfcGpu.apcm_encode returns them), stored behind frame.json as radio-<id>.apcm with the id of their header."""
    content = json.dumps({"frames": [frame_entry(f, stream_time) for f in frames]}).encode("ascii")
    with tarfile.open(path, "w:gz", compresslevel=9, format=tarfile.USTAR_FORMAT) as tar:
        info = tarfile.TarInfo("frame.json")
        info.size = len(content)
        info.mode = 0o664
        tar.addfile(info, io.BytesIO(content))
        for entry in signals or ():
            entry = bytes(entry)
            info = tarfile.TarInfo("radio-%d.apcm" % struct.unpack_from("<I", entry, 20)[0])
            info.size = len(entry)
            info.mode = 0o664
            tar.addfile(info, io.BytesIO(entry))
    return len(content)


def parse_apcm(entry):
    """(header, values int16, offsets uint32) of an APCM entry as TraceStorageTask::readRadioEntry takes it (:760-879): the
    header is {"version", "info": the six words, "stream_id", "sample_rate", "samples"}; the records' deltas are summed mod 2^16
    and mod 2^32 from the header's start offset (info[1]). The reference's reader restarts its offsets with every chunk of 16 384
    records and adds the chunk's last one to the next chunk's position, which is the same sum. ValueError for what that reader
    refuses: another magic or version, a size that is not 32 + 3 * samples."""
    import numpy as np
    entry = bytes(entry)
    if len(entry) < 32 or entry[:4] != b"APCM":
        raise ValueError("not an APCM entry")
    version, *info = struct.unpack_from("<7I", entry, 4)
    if version != 2:
        raise ValueError("APCM version %d" % version)
    if len(entry) != 32 + 3 * info[2]:
        raise ValueError("APCM entry of %d bytes with %d samples" % (len(entry), info[2]))
    raw = np.frombuffer(entry, dtype=np.uint8, offset=32).reshape(-1, 3).astype(np.uint32)
    offsets = (info[1] + np.cumsum(raw[:, 0], dtype=np.uint64)).astype(np.uint32)
    values = np.cumsum(raw[:, 1] | (raw[:, 2] << 8), dtype=np.uint64).astype(np.uint16).view(np.int16)
    header = {"version": version, "info": tuple(info), "stream_id": info[3], "sample_rate": info[4], "samples": info[2]}
    return header, values, offsets


def read_trz_signal(path):
    """{stream id: (header, values int16, offsets uint32)} of the radio-<id>.apcm entries of a trace, stored or deflated."""
    signals = {}
    with tarfile.open(path, "r:gz") as tar:
        for member in tar:
            if member.isfile() and member.name.startswith("radio-") and member.name.endswith(".apcm"):
                header, values, offsets = parse_apcm(tar.extractfile(member).read())
                signals[header["stream_id"]] = (header, values, offsets)
    return signals


def write_trz_per_stream(directory, frames_by_stream, stream_time=0.0, prefix="stream"):
    """One trace per stream of a batch run ({stream id: [frames]}, as frames.parse_sink returns); returns the paths."""
    import os
    paths = []
    for sid in sorted(frames_by_stream):
        path = os.path.join(directory, "%s_%06d.trz" % (prefix, sid))
        write_trz(path, frames_by_stream[sid], stream_time)
        paths.append(path)
    return paths
