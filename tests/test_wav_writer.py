"""nfcgpu_wav_write / nfcgpu_wav_append: the capture file hw::RecordDevice writes (RecordDevice.cpp:493-546), host only -
no context, no device. The header is checked field by field here; tests/test_record.py compares whole files with what
the reference wrote."""
import os
import struct

import numpy as np
import pytest

EINVAL, EIO = -1, -9
FS = 10000000


@pytest.fixture(scope="module")
def wav(built):
    import nfclab_amd
    nfclab_amd.load_library()
    return nfclab_amd


def header_of(raw):
    fields = struct.unpack("<4sI4s4sIHHIIHH4sI4sI8i4sI", raw[:92])
    names = ("riff", "riff_size", "wave", "fmt", "fmt_size", "format", "channels", "rate", "byte_rate", "block_align", "bits", "meta_chunk",
             "meta_size", "meta", "epoch")
    h = dict(zip(names, fields[:15]))
    h["keys"], h["data"], h["data_size"] = list(fields[15:23]), fields[23], fields[24]
    return h


@pytest.mark.parametrize("channels", [1, 2, 8])
def test_the_header_is_the_92_bytes_of_the_reference(wav, tmp_path, channels):
    rng = np.random.default_rng(channels)
    pcm = rng.integers(-32768, 32768, (1001, channels)).astype(np.int16)
    keys = [7 * (c + 1) * (-1) ** c for c in range(channels)]
    path = str(tmp_path / "a.wav")
    wav.wav_write(path, pcm, FS, channels=channels, stream_time=1760000000, keys=keys)
    raw = open(path, "rb").read()
    assert len(raw) == 92 + pcm.size * 2
    assert header_of(raw) == {"riff": b"RIFF", "riff_size": len(raw) - 8, "wave": b"WAVE", "fmt": b"fmt ", "fmt_size": 16, "format": 1,
                              "channels": channels, "rate": FS, "byte_rate": FS * channels * 2, "block_align": channels * 2, "bits": 16,
                              "meta_chunk": b"META", "meta_size": 40, "meta": b"meta", "epoch": 1760000000,
                              "keys": keys + [0] * (8 - channels), "data": b"data", "data_size": len(raw) - 92}
    assert np.array_equal(np.frombuffer(raw[92:], dtype="<i2").reshape(-1, channels), pcm)
    # keys = None: zeros
    wav.wav_write(path, pcm, FS, channels=channels)
    assert header_of(open(path, "rb").read())["keys"] == [0] * 8


def test_append_adds_samples_and_rewrites_both_sizes(wav, tmp_path):
    rng = np.random.default_rng(3)
    pcm = rng.integers(-32768, 32768, (70000, 2)).astype(np.int16)
    whole, pieces = str(tmp_path / "whole.wav"), str(tmp_path / "pieces.wav")
    wav.wav_write(whole, pcm, FS, channels=2, stream_time=5, keys=[1, 2])
    wav.wav_write(pieces, pcm[:0], FS, channels=2, stream_time=5, keys=[1, 2])
    assert os.path.getsize(pieces) == 92 and header_of(open(pieces, "rb").read())["data_size"] == 0
    at = 0
    for count in (1, 0, 33000, 36999):
        wav.wav_append(pieces, pcm[at:at + count])
        at += count
        h = header_of(open(pieces, "rb").read())
        assert h["data_size"] == at * 4 and h["riff_size"] == 92 + at * 4 - 8
    assert open(pieces, "rb").read() == open(whole, "rb").read()


def test_refusals(wav, tmp_path):
    lib = wav.load_library()
    pcm = np.arange(16, dtype=np.int16)
    path = os.fsencode(str(tmp_path / "r.wav"))
    assert lib.nfcgpu_wav_write(None, pcm.ctypes.data, 16, 1, FS, 0, None) == EINVAL
    assert lib.nfcgpu_wav_write(path, pcm.ctypes.data, 16, 0, FS, 0, None) == EINVAL
    assert lib.nfcgpu_wav_write(path, pcm.ctypes.data, 2, 9, FS, 0, None) == EINVAL
    assert lib.nfcgpu_wav_write(path, None, 16, 1, FS, 0, None) == EINVAL
    # a file that would pass 4 GiB is refused before anything is opened
    assert lib.nfcgpu_wav_write(path, pcm.ctypes.data, (1 << 31) - 40, 1, FS, 0, None) == EINVAL
    assert not os.path.exists(path)
    assert lib.nfcgpu_wav_write(os.fsencode(str(tmp_path / "no" / "such" / "dir.wav")), pcm.ctypes.data, 16, 1, FS, 0, None) == EIO
    assert lib.nfcgpu_wav_append(os.fsencode(str(tmp_path / "absent.wav")), pcm.ctypes.data, 16) == EIO
    assert lib.nfcgpu_wav_append(None, pcm.ctypes.data, 16) == EINVAL

    # appending to files without that header: a plain 44-byte WAV, a short file, a header whose sizes do not match the file
    plain = str(tmp_path / "plain.wav")
    raw = pcm.tobytes() * 8
    with open(plain, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + len(raw)) + b"WAVE" + b"fmt " + struct.pack("<IHHIIHH", 16, 1, 1, FS, FS * 2, 2, 16))
        f.write(b"data" + struct.pack("<I", len(raw)) + raw)
    before = open(plain, "rb").read()
    assert lib.nfcgpu_wav_append(os.fsencode(plain), pcm.ctypes.data, 16) == EINVAL
    assert open(plain, "rb").read() == before
    short = str(tmp_path / "short.wav")
    open(short, "wb").write(b"RIFF")
    assert lib.nfcgpu_wav_append(os.fsencode(short), pcm.ctypes.data, 16) == EINVAL
    cut = str(tmp_path / "cut.wav")
    wav.wav_write(cut, pcm, FS)
    open(cut, "ab").write(b"\0\0")
    assert lib.nfcgpu_wav_append(os.fsencode(cut), pcm.ctypes.data, 16) == EINVAL
    with pytest.raises(wav.NfcGpuError):
        wav.wav_append(cut, pcm)
