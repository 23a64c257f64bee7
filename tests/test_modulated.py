"""Modulated exchanges that no capture holds (tests/modulated_cases.py, built by tests/nfc_modem.py) on the CPU: the reference
decoder recovers what was modulated - so the other tests of these streams do not pass on empty lists - and the CPU step machine
(tests/hostsim) decodes every stream exactly as the reference does. The yardstick is the live reference on the same float32
samples, all nine fields of every frame, carrier frames included."""
import functools

import pytest

import modulated_cases as C
import nfc_modem as M
import nfc_testlib as T

needs_reference = pytest.mark.skipif(T.reference_lib() is None, reason="oracle/_ref not built")

HOST = [c for c in C.CASES if c.where != "device"]           # the scenario for FWI 14 is built for the device alone
CLAIMED = [c for c in HOST if c.group != 5]                  # the weak-signal sweeps claim nothing about what is decoded

# Scenarios of which the reference does not recover what was sent, and what it does instead. Not more than a tenth of the scenarios
# of groups 1-4, and each of them has to stay one: test_the_exceptions_are_few_and_still_exceptions.
EXCEPTIONS = {
    "b212 with answers": "the reference reports the two requests at 211 875 and no answer: its NFC-B answer search runs at the rate of the request and finds no start of frame at 212 kbps",
    "b424": "the reference reports nothing: its NFC-B request detector tries 106 and 212 kbps only",
    "a106 with answers at 2.5 MS/s": "the reference reports ATQA and garbles the longer answers (tried: load 0.1 - 0.7, smoothing of 100 and 300 ns, edges on "
                                     "whole samples; a capture decimated to 2.5 MS/s loses answers too): an eighth of a bit is under three samples there",
}

FLAG = {"none": 0x00, "ciphered": 0x00, "parity": 0x10, "crc": 0x20, "sync": 0x40}
DEFECTS = 0x78                                               # lab::FrameFlags Truncated, ParityError, CrcError, SyncError


@functools.lru_cache(maxsize=2)
def stream(name):
    x, sent = C.build(name)
    ref, _ = T.reference_decode(x, sample_rate=C.BY_NAME[name].fs, keep_carrier=True, cap=16384, defined_storage=True)
    return x, sent, ref


def complaints(sent, ref):
    """What keeps the reference's data frames from being `sent`. Every data frame has to begin inside a burst that was sent, and
    - a burst sent whole (defect none, parity, crc, sync) gives exactly one frame with its technology, direction, rate and bytes
      and with that defect's flag alone among the four defect flags; a ciphered one (after a Mifare AUTH) gives its bytes with the
      flag Encrypted and no defect flag;
    - an oversize burst gives exactly one frame flagged Truncated that holds a proper prefix of its bytes;
    - a truncated burst gives nothing or one frame that agrees with the bytes sent whole before the cut (the byte that was cut may
      follow, and the last whole byte may be missing: the decoders take a byte when the symbol after it has been seen);
    - a late answer gives nothing, and so does what is sent after an NFC-B answer that broke off (modulated_cases.unheard); an early one gives nothing or any frame but the intact one.
    The rate of an NFC-V answer is not compared: the reference labels it with the rate of the request's coding."""
    out = []
    frames = {i: [] for i in range(len(sent))}
    for f in ref:
        if f[1] not in (M.POLL, M.LISTEN):
            continue
        at = [i for i, s in enumerate(sent) if s.start - 64 <= f[5] <= s.end]
        if len(at) != 1:
            out.append("a frame where nothing was sent: " + T.describe(f))
        else:
            frames[at[0]].append(f)
    for i, s in enumerate(sent):
        what = "burst %d (%x %x %d %s, %d bytes)" % (i, s.tech, s.type, s.rate, s.defect, len(s.data))
        got = frames[i]
        same = [f for f in got if f[0] == s.tech and f[1] == s.type and (f[4] == s.rate or (s.tech == M.TECH_V and s.type == M.LISTEN))]
        if len(same) != len(got):
            out.append(what + ": a frame of another technology, direction or rate")
        elif s.defect in FLAG:
            if len(got) != 1 or got[0][8] != s.data or got[0][2] & DEFECTS != FLAG[s.defect] or bool(got[0][2] & 0x02) != (s.defect == "ciphered"):
                out.append(what + ": " + ("; ".join(T.describe(f) for f in got) or "no frame"))
        elif s.defect == "oversize":
            if len(got) != 1 or not got[0][2] & 0x08 or not (0 < len(got[0][8]) < len(s.data)) or s.data[:len(got[0][8])] != got[0][8]:
                out.append(what + ": " + ("; ".join(T.describe(f) for f in got) or "no frame"))
        elif s.defect == "truncated":
            for f in got:
                n = min(len(f[8]), len(s.data) - 1)
                if len(got) > 1 or len(f[8]) > len(s.data) + 1 or len(f[8]) < len(s.data) - 1 or f[8][:n] != s.data[:n]:
                    out.append(what + ": " + T.describe(f))
        elif s.defect in ("late", "unheard"):
            if got:
                out.append(what + ": " + T.describe(got[0]))
        elif s.defect == "early":
            if any(f[8] == s.data and not f[2] & DEFECTS for f in got):
                out.append(what + ": reported intact")
        else:
            out.append(what + ": unknown defect")
    return out


@needs_reference
@pytest.mark.parametrize("name", [c.name for c in CLAIMED if c.name not in EXCEPTIONS])
def test_reference_recovers_what_was_modulated(name):
    x, sent, ref = stream(name)
    assert sent and complaints(sent, ref) == []


@needs_reference
def test_the_exceptions_are_few_and_still_exceptions():
    assert set(EXCEPTIONS) <= {c.name for c in CLAIMED}
    assert 10 * len(EXCEPTIONS) <= sum(c.group <= 4 for c in C.CASES)
    for name in EXCEPTIONS:
        x, sent, ref = stream(name)
        assert complaints(sent, ref) != [], name + " is decoded now: take it off the list"


@needs_reference
def test_the_table_reaches_what_it_exists_for():
    """On the reference's output alone: every defect flag of lab::FrameFlags (Truncated 0x08, ParityError 0x10, CrcError 0x20,
    SyncError 0x40) on every technology that can raise it, and the modes no capture holds. ParityError is NFC-A's alone (no other
    technology has parity bits) and SyncError NFC-F's (NfcF.cpp:467-472 and 597-602 are the only places that set it)."""
    flags = {t: 0 for t in (M.TECH_A, M.TECH_B, M.TECH_F, M.TECH_V)}
    seen = set()
    longest = {}
    for c in CLAIMED:
        x, sent, ref = stream(c.name)
        for f in ref:
            if f[1] in (M.POLL, M.LISTEN):
                flags[f[0]] |= f[2]
                seen.add((f[0], f[1], f[4]))
                longest[f[0], f[1]] = max(longest.get((f[0], f[1]), 0), len(f[8]))
    assert flags[M.TECH_A] & 0x7B == 0x3B, hex(flags[M.TECH_A])      # short, encrypted, truncated, parity, CRC
    assert flags[M.TECH_B] & 0x78 == 0x28, hex(flags[M.TECH_B])
    assert flags[M.TECH_F] & 0x78 == 0x68, hex(flags[M.TECH_F])
    assert flags[M.TECH_V] & 0x78 == 0x28, hex(flags[M.TECH_V])
    for tech, rates in ((M.TECH_A, (105938, 211875, 423750)), (M.TECH_F, (211875, 423750)), (M.TECH_V, (26484, 1655))):
        for rate in rates:
            assert (tech, M.POLL, rate) in seen and (tech, M.LISTEN, rate) in seen, (hex(tech), rate)
    assert (M.TECH_B, M.POLL, 211875) in seen and (M.TECH_B, M.POLL, 105938) in seen and (M.TECH_B, M.LISTEN, 105938) in seen
    for key in ((M.TECH_A, M.POLL), (M.TECH_A, M.LISTEN), (M.TECH_B, M.POLL), (M.TECH_B, M.LISTEN), (M.TECH_F, M.POLL), (M.TECH_F, M.LISTEN)):
        assert longest[key] >= 250, (key, longest[key])
    assert longest[M.TECH_V, M.POLL] >= 64 and longest[M.TECH_V, M.LISTEN] >= 64, longest


def test_the_table_is_fixed_and_seeded():
    """the same call gives the same samples; every group is there, every technology in the groups 1, 2, 3 and 5"""
    import numpy as np
    a, _ = C.build("a106 wrong parity")
    b, _ = C.build("a106 wrong parity")
    assert np.array_equal(a, b)
    g, _ = C.build("a106 wrong parity", grid=True)
    assert np.array_equal(g, np.round(g * 32768) / 32768) and not np.array_equal(a, g)
    assert {c.group for c in C.CASES} == {1, 2, 3, 4, 5, 6}
    for group in (1, 2, 3, 5):
        for tech in "abfv":
            if (group, tech) != (3, "v"):     # nfcv_process branches on nothing but the CRC: group 2 has that
                assert any(c.group == group and (c.name.startswith(tech) or c.name.startswith("weak " + tech)) for c in C.CASES), (group, tech)


@needs_reference
@pytest.mark.parametrize("name", [c.name for c in HOST])
def test_step_machine_matches_reference_on_modulated_exchanges(built, name):
    x, sent, ref = stream(name)
    assert T.hostsim_decode(x, sample_rate=C.BY_NAME[name].fs, keep_carrier=True, cap=16384, lane=len(name) % 64) == ref
    assert len(ref) > 0
