"""A small baseband modulator for the decode tests: NFC-A, -B, -F and -V frames in both directions as the magnitude signal
a decoder sees after IQ -> magnitude, written from the air-interface standards (ISO/IEC 14443-2/-3 types A and B,
JIS X 6319-4 / ISO/IEC 18092 for F, ISO/IEC 15693-2/-3 for V). Test infrastructure, numpy only.

All times are in carrier cycles (1 / 13.56 MHz), so one description of a frame serves every sample rate. A frame is a
Burst: a table of (from, to, delta) rows - between `from` and `to` the carrier is multiplied by (1 + the sum of the deltas
that cover the sample) - plus what it carries (Sent). exchange() strings bursts on one continuous carrier.

    x, sent = exchange([nfca_poll(b"\\x26", bits7=True), nfca_listen(b"\\x04\\x00", crc=False)])
"""
import collections

import numpy as np

FC = 13.56e6
TECH_A, TECH_B, TECH_F, TECH_V = 0x101, 0x102, 0x103, 0x104
POLL, LISTEN = 0x102, 0x103

# what was modulated: technology, direction, symbols per second, the bytes on the air (CRC included, as sent: a CRC made wrong
# is listed wrong) and the defect put into it: "none", "parity", "crc", "sync" (NFC-F), "truncated" (data: the bytes sent
# whole before the cut). A scenario may relabel a burst (Burst.sent._replace(defect=...)) where the defect lies in its place
# in the exchange and not in its signal: "early" / "late" (an answer outside the window in which a reader listens),
# "oversize" (longer than the frame size the exchange agreed on)
# start, end: the burst's first and last sample in the stream (filled in by exchange())
Sent = collections.namedtuple("Sent", "tech type rate data defect start end", defaults=(None, None))
Burst = collections.namedtuple("Burst", "segs length sent gap cut_mode")


# ---------------------------------------------------------------------------------------------------- checksums

def crc_a(data):
    """CRC_A (ISO/IEC 14443-3 annex B): reflected 0x1021, preset 0x6363, not inverted, low byte first"""
    crc = 0x6363
    for b in data:
        crc ^= b
        for _ in range(8):
            crc = (crc >> 1) ^ 0x8408 if crc & 1 else crc >> 1
    return bytes([crc & 0xFF, crc >> 8])


def crc_b(data):
    """CRC_B (ISO/IEC 14443-3 annex B) and the CRC of ISO/IEC 15693: reflected 0x1021, preset 0xFFFF, inverted, low byte first"""
    crc = 0xFFFF
    for b in data:
        crc ^= b
        for _ in range(8):
            crc = (crc >> 1) ^ 0x8408 if crc & 1 else crc >> 1
    crc ^= 0xFFFF
    return bytes([crc & 0xFF, crc >> 8])


def crc_f(data):
    """CRC of NFC-F frames (JIS X 6319-4): 0x1021, preset 0, high byte first"""
    crc = 0
    for b in data:
        crc ^= b << 8
        for _ in range(8):
            crc = ((crc << 1) ^ 0x1021) & 0xFFFF if crc & 0x8000 else (crc << 1) & 0xFFFF
    return bytes([crc >> 8, crc & 0xFF])


def _with_crc(data, crc, fn, bad_crc):
    data = bytes(data)
    if not crc:
        return data
    c = fn(data)
    if bad_crc:
        c = bytes([c[0] ^ 0x5A, c[1]])
    return data + c


# ---------------------------------------------------------------------------------------------------- pieces of a frame

def _burst(t0, halves, half, lo, hi=0.0, low_first=True):
    """rows of a square subcarrier: `halves` half cycles of `half` carrier cycles from t0, the low ones at 1 + lo, the high ones at
    1 + hi (a row is left out where the delta is 0)"""
    rows = []
    for k in range(halves):
        d = lo if (k % 2 == 0) == low_first else hi
        if d:
            rows.append((t0 + k * half, t0 + (k + 1) * half, d))
    return rows


def _finish(symbols, cut, sent, gap, cut_mode, whole_bytes=None):
    """symbols: list of (duration, rows relative to the symbol's start). cut: keep that many symbols only (the frame is then
    listed as truncated with the bytes in `whole_bytes(cut)`)"""
    if cut is not None and cut < len(symbols):
        symbols = symbols[:cut]
        sent = sent._replace(defect="truncated", data=whole_bytes(cut) if whole_bytes else b"")
    else:
        cut_mode = None
    rows, t = [], 0.0
    for dur, sym in symbols:
        rows += [(t + a, t + b, d) for a, b, d in sym]
        t += dur
    return Burst(np.array(rows, dtype=np.float64).reshape(-1, 3), t, sent, gap, cut_mode)


def _rate_index(rate, allowed=(106, 212, 424)):
    assert rate in allowed, rate
    return (106, 212, 424, 848).index(rate)


def _sps(cycles_per_symbol):
    return int(FC / cycles_per_symbol + 0.5)


# ---------------------------------------------------------------------------------------------------- NFC-A

def _bits_a(data, bits7, bad_parity, last_parity_inverted=False):
    """bytes LSB first, each followed by an odd parity bit (ISO/IEC 14443-3 6.2.3); a short frame is 7 bits without parity"""
    if bits7:
        return [(data[0] >> i) & 1 for i in range(7)]
    bits = []
    for k, b in enumerate(data):
        p = 1 ^ (bin(b).count("1") & 1)
        if bad_parity is not None and k == bad_parity:
            p ^= 1
        if last_parity_inverted and k == len(data) - 1:
            p ^= 1
        bits += [(b >> i) & 1 for i in range(8)] + [p]
    return bits


def nfca_poll(data, rate=106, bits7=False, crc=True, bad_crc=False, bad_parity=None, cut=None, cut_mode="stop",
              depth=0.95, pause=None, gap=20000):
    """Reader frame of type A: modified Miller (ISO/IEC 14443-2 8.1): X = pause in the second half of the bit, Y = no pause,
    Z = pause at its start; start of communication Z, `1` = X, `0` = Y after a `1` and Z otherwise, end = `0` then Y. The pause
    is `pause` carrier cycles at 1 - depth (default 38 cycles = 2.8 us at 106 kbps and in proportion at 212 / 424)."""
    r = _rate_index(rate)
    etu = 128 >> r
    pause = pause if pause is not None else 38.0 / (1 << r)
    data = _with_crc(data, crc and not bits7, crc_a, bad_crc)
    bits = _bits_a(data, bits7, bad_parity)
    X, Y, Z = [(etu / 2, etu / 2 + pause, -depth)], [], [(0.0, pause, -depth)]
    symbols, prev = [(etu, Z)], 0
    for b in bits + [0]:
        symbols.append((etu, X if b else (Y if prev else Z)))
        prev = b
    symbols.append((etu, Y))
    defect = "parity" if bad_parity is not None else "crc" if bad_crc else "none"
    return _finish(symbols, cut, Sent(TECH_A, POLL, _sps(etu), data, defect), gap, cut_mode,
                   lambda n: data[:max(0, n - 1) // 9])


def nfca_listen(data, rate=106, bits7=False, crc=True, bad_crc=False, bad_parity=None, cut=None, cut_mode="stop",
                load=0.2, gap=1085):
    """Card frame of type A (ISO/IEC 14443-2 8.2). 106 kbps: Manchester on the 847.5 kHz subcarrier - subcarrier in the first
    half of the bit for start and `1`, in the second half for `0`, none at the end. 212 / 424 kbps: BPSK of the subcarrier, NRZ-L:
    32 subcarrier cycles of the `1` phase, one bit of the inverted phase as start, the bits, then no subcarrier; the last
    parity bit is inverted (14443-3 6.2.3.2.2). The card's load pulls the carrier to 1 - load in the low half of a subcarrier
    cycle. A short frame here is the 4-bit answer of a Mifare card (ACK / NAK)."""
    r = _rate_index(rate)
    etu = 128 >> r
    data = _with_crc(data, crc and not bits7, crc_a, bad_crc)
    if bits7:
        bits = [(data[0] >> i) & 1 for i in range(4)]
    else:
        bits = _bits_a(data, False, bad_parity, last_parity_inverted=(r > 0))
    symbols = []
    if r == 0:
        D = _burst(0.0, 8, 8, -load)
        E = _burst(etu / 2, 8, 8, -load)
        symbols.append((etu, D))
        symbols += [(etu, D if b else E) for b in bits]
        symbols.append((etu, []))
        whole = lambda n: data[:max(0, n - 1) // 9]
    else:
        per = etu // 8                                   # half cycles of the subcarrier in one bit
        symbols.append((32 * 16, _burst(0.0, 64, 8, -load)))
        symbols.append((etu, _burst(0.0, per, 8, -load, low_first=False)))
        symbols += [(etu, _burst(0.0, per, 8, -load, low_first=bool(b))) for b in bits]
        whole = lambda n: data[:max(0, n - 2) // 9]
    defect = "parity" if bad_parity is not None else "crc" if bad_crc else "none"
    return _finish(symbols, cut, Sent(TECH_A, LISTEN, _sps(etu), data, defect), gap, cut_mode, whole)


# ---------------------------------------------------------------------------------------------------- NFC-B

def _chars_b(data):
    """start of frame (10 etu `0`, 2 etu `1`), a character per byte (start bit `0`, 8 bits LSB first, stop bit `1`), end of frame
    (10 etu `0`): ISO/IEC 14443-3 7.1"""
    bits = [0] * 10 + [1] * 2
    for b in data:
        bits += [0] + [(b >> i) & 1 for i in range(8)] + [1]
    return bits + [0] * 10


def nfcb_poll(data, rate=106, crc=True, bad_crc=False, cut=None, cut_mode="stop", depth=0.5, gap=20000):
    """Reader frame of type B: NRZ-L amplitude shift keying, the carrier at 1 - depth during a `0` (ISO/IEC 14443-2 9.1)"""
    r = _rate_index(rate)
    etu = 128 >> r
    data = _with_crc(data, crc, crc_b, bad_crc)
    symbols = [(etu, [] if b else [(0.0, etu, -depth)]) for b in _chars_b(data)]
    return _finish(symbols, cut, Sent(TECH_B, POLL, _sps(etu), data, "crc" if bad_crc else "none"), gap, cut_mode,
                   lambda n: data[:max(0, n - 12) // 10])


def nfcb_listen(data, rate=106, crc=True, bad_crc=False, cut=None, cut_mode="stop", load=0.25, tr1=80, gap=2712):
    """Card frame of type B: BPSK of the 847.5 kHz subcarrier, NRZ-L (ISO/IEC 14443-2 9.2): `tr1` subcarrier cycles unmodulated,
    the frame with `0` as the inverted phase, one etu of the `1` phase to close. The carrier swings to 1 +- load."""
    r = _rate_index(rate)
    etu = 128 >> r
    data = _with_crc(data, crc, crc_b, bad_crc)
    per = etu // 8
    symbols = [(tr1 * 16, _burst(0.0, 2 * tr1, 8, -load, load))]
    symbols += [(etu, _burst(0.0, per, 8, -load, load, low_first=bool(b))) for b in _chars_b(data) + [1]]
    return _finish(symbols, cut, Sent(TECH_B, LISTEN, _sps(etu), data, "crc" if bad_crc else "none"), gap, cut_mode,
                   lambda n: data[:max(0, n - 13) // 10])


# ---------------------------------------------------------------------------------------------------- NFC-F

SYNC_F = b"\xB2\x4D"


def _nfcf(data, rate, listen, crc, bad_crc, reversed_polarity, cut, cut_mode, depth, gap, preamble, sync):
    r = _rate_index(rate, (212, 424))
    etu = 128 >> r
    body = bytes([len(data) + 1]) + bytes(data)
    body = _with_crc(body, crc, crc_f, bad_crc)
    raw = bytes(preamble) + sync + body
    first, second = [(0.0, etu / 2, -depth)], [(etu / 2, etu, -depth)]
    if reversed_polarity:
        first, second = second, first
    symbols = []
    for b in raw:
        symbols += [(etu, second if (b >> i) & 1 else first) for i in range(7, -1, -1)]
    sent = Sent(TECH_F, LISTEN if listen else POLL, _sps(etu), body, "sync" if sync != SYNC_F else "crc" if bad_crc else "none")
    return _finish(symbols, cut, sent, gap, cut_mode, lambda n: body[:max(0, n // 8 - preamble - 2)])


def nfcf_poll(data, rate=212, crc=True, bad_crc=False, reversed_polarity=False, cut=None, cut_mode="stop", depth=0.45, gap=20000,
              preamble=6, sync=SYNC_F):
    """Reader frame of NFC-F (JIS X 6319-4): `preamble` zero bytes, sync B2 4D, length (itself included), payload, CRC; Manchester,
    MSB first: a `0` has the carrier at 1 - depth in the first half of the bit, a `1` in the second half (the other way round
    with reversed_polarity: the standard admits both). sync: other bytes in place of B2 4D are a defect"""
    return _nfcf(data, rate, False, crc, bad_crc, reversed_polarity, cut, cut_mode, depth, gap, preamble, sync)


def nfcf_listen(data, rate=212, crc=True, bad_crc=False, reversed_polarity=False, cut=None, cut_mode="stop", depth=0.25, gap=35256,
                preamble=6, sync=SYNC_F):
    """Card frame of NFC-F: the same coding as the reader's, by load modulation without a subcarrier"""
    return _nfcf(data, rate, True, crc, bad_crc, reversed_polarity, cut, cut_mode, depth, gap, preamble, sync)


# ---------------------------------------------------------------------------------------------------- NFC-V

def nfcv_poll(data, mode=4, crc=True, bad_crc=False, cut=None, cut_mode="stop", depth=0.97, gap=20000):
    """Reader frame of ISO/IEC 15693-2: pulse-position coding with pauses of 9.44 us (128 carrier cycles): start of frame,
    the bytes in 1-of-4 (mode 4: two bits per 75.52 us slot group, low pair first) or 1-of-256 coding (mode 256), end of frame"""
    unit = 128.0
    data = _with_crc(data, crc, crc_b, bad_crc)
    P = lambda k: (k * unit, (k + 1) * unit, -depth)
    symbols = [(8 * unit, [P(0), P(7)] if mode == 256 else [P(0), P(5)])]
    for b in data:
        if mode == 256:
            symbols.append((512 * unit, [P(2 * b + 1)]))
        else:
            symbols += [(8 * unit, [P(2 * ((b >> (2 * k)) & 3) + 1)]) for k in range(4)]
    symbols.append((4 * unit, [P(2)]))
    per_byte = 1 if mode == 256 else 4
    return _finish(symbols, cut, Sent(TECH_V, POLL, _sps(512 if mode == 4 else 8192), data, "crc" if bad_crc else "none"), gap, cut_mode,
                   lambda n: data[:max(0, n - 1) // per_byte])


def nfcv_listen(data, crc=True, bad_crc=False, cut=None, cut_mode="stop", load=0.2, gap=4352):
    """Card frame of ISO/IEC 15693-2, one subcarrier (fc / 32), high data rate: a bit is 512 carrier cycles, `0` = 8 subcarrier
    pulses then nothing, `1` = nothing then 8 pulses; start = 768 cycles unmodulated, 24 pulses, a `1`; end = a `0`, 24 pulses,
    768 cycles unmodulated; bytes LSB first"""
    data = _with_crc(data, crc, crc_b, bad_crc)
    zero, one = _burst(0.0, 16, 16, -load), _burst(256.0, 16, 16, -load)
    symbols = [(1536 + 512, _burst(768.0, 48, 16, -load) + [(a + 1536, b + 1536, d) for a, b, d in one])]
    for b in data:
        symbols += [(512, one if (b >> i) & 1 else zero) for i in range(8)]
    symbols.append((512 + 1536, zero + _burst(512.0, 48, 16, -load)))
    return _finish(symbols, cut, Sent(TECH_V, LISTEN, _sps(512), data, "crc" if bad_crc else "none"), gap, cut_mode,
                   lambda n: data[:max(0, n - 1) // 8])


def synth_nfcv_poll(payload, mode, lead=30000, tail=60000, level=0.5, depth=0.97, noise=0.0005, seed=1, sample_rate=10000000):
    """Synthetic ISO 15693 reader frame (pulse-position coding, 9.44 us pauses): SOF, `payload` in 1-of-4 (mode 4) or
    1-of-256 (mode 256) coding, EOF, on an unmodulated carrier. No fixture of the reference uses 1-of-256."""
    unit = 9.44e-6 * sample_rate           # one half slot
    pauses = [(0, 1), (7, 8)] if mode == 256 else [(0, 1), (5, 6)]
    t = 8
    for b in payload:
        if mode == 256:
            pauses.append((t + 2 * b + 1, t + 2 * b + 2))
            t += 512
        else:
            for k in range(4):
                v = (b >> (2 * k)) & 3
                pauses.append((t + 2 * v + 1, t + 2 * v + 2))
                t += 8
    pauses.append((t + 2, t + 3))
    t += 4
    x = np.full(int(lead + t * unit + tail), level, np.float32)
    for a, b in pauses:
        x[int(round(lead + a * unit)):int(round(lead + b * unit))] = level * (1 - depth)
    x = np.convolve(x, np.array([0.25, 0.5, 0.25], np.float32), mode="same").astype(np.float32)
    x += np.random.default_rng(seed).normal(0, noise, x.size).astype(np.float32)
    x[:200] *= np.linspace(0, 1, 200, dtype=np.float32)
    return x


# ---------------------------------------------------------------------------------------------------- the stream

def quiet(cycles):
    """unmodulated carrier for that many carrier cycles"""
    return ("quiet", float(cycles))


def carrier_off(cycles):
    """no carrier for that many carrier cycles"""
    return ("off", float(cycles))


def exchange(items, fs=10000000, level=0.3, smooth=3, noise=0.0005, seed=1, ppm=0.0, grid=False, lead=13560, tail=27120,
             max_samples=None, oversample=4):
    """One stream: `lead` cycles of carrier, the items (bursts, each after its own `gap` of quiet carrier; quiet(); carrier_off())
    and `tail` cycles of carrier. level: the unmodulated carrier; smooth: length of the box filter over the edges in units of 100 ns
    (three: the three taps at 10 MS/s of the captures' look); noise: sigma of
    the white noise added (numpy.random.default_rng(seed)); ppm: error of the symbol clock of every burst; grid: round onto the
    int16 grid of a capture. A burst cut with cut_mode "off" is followed by 5000 cycles without carrier, one cut with "end" ends
    the stream. max_samples: the stream is cut there. The edges are placed and smoothed on a time grid `oversample` times finer
    than the samples, of which every `oversample`-th value is taken (at 2.5 MS/s a subcarrier cycle is under three samples: edges on
    whole samples, or a filter as long as three of them, leave nothing of it). Returns (float32 samples, [Sent of every burst])."""
    spc = oversample * fs / FC
    rows, sent, t = [], [], float(lead)
    for it in items:
        if isinstance(it, tuple) and not isinstance(it, Burst):
            if it[0] == "off":
                rows.append(np.array([[t, t + it[1], -1.0]]))
            t += it[1]
            continue
        t += it.gap
        if len(it.segs):
            seg = it.segs.copy()
            seg[:, :2] = t + seg[:, :2] * (1 + ppm * 1e-6)
            rows.append(seg)
        sent.append(it.sent._replace(start=int(t * spc) // oversample, end=int((t + it.length * (1 + ppm * 1e-6)) * spc) // oversample))
        t += it.length * (1 + ppm * 1e-6)
        if it.cut_mode == "off":
            rows.append(np.array([[t, t + 5000.0, -1.0]]))
            t += 5000.0
        elif it.cut_mode == "end":
            tail = 0
            break
    total = int(round((t + tail) * spc / oversample)) * oversample
    d = np.zeros(total + 2, dtype=np.float64)
    if rows:
        seg = np.concatenate(rows)
        a = np.clip(np.rint(seg[:, 0] * spc).astype(np.int64), 0, total)
        b = np.clip(np.rint(seg[:, 1] * spc).astype(np.int64), 0, total)
        np.add.at(d, a, seg[:, 2])
        np.add.at(d, b, -seg[:, 2])
    x = level * (1.0 + np.cumsum(d)[:total])
    box = int(round(smooth * 1e-7 * fs * oversample))
    if box > 1:
        x = np.convolve(x, np.full(box, 1.0 / box), mode="same")
    x = x[::oversample]
    total //= oversample
    if noise:
        x = x + np.random.default_rng(seed).normal(0.0, noise, total)
    x = np.abs(x)
    if grid:
        x = np.round(x * 32768.0) / 32768.0
    if max_samples is not None:
        x = x[:max_samples]
    return x.astype(np.float32), sent
