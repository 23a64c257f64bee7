"""The scenario table of the modulated-exchange tests: exchanges that no capture holds, built by tests/nfc_modem.py.
A fixed, seeded list; every entry is a name, its group, the sample rate, and the call that builds the items of the exchange.

groups: 1 every (technology, rate, direction), short and long frames; 2 defects; 3 protocol feedback; 4 technologies after one
another; 5 weak signals (a sweep of depth / load from clearly decodable down to nothing); 6 groups 1-4 at 5 and 2.5 MS/s.

where: "all" every leg; "step" too long for the emulated runtime (the reference, the CPU step machine and the device take it);
"device" only the device legs take it."""
import collections

import nfc_modem as M

Case = collections.namedtuple("Case", "name group fs items kw where")

FS = 10000000
PAY = bytes((37 * i + 11 + i // 256) & 0xFF for i in range(600))   # frame contents: any bytes will do (requests from the front, answers from 300 on)
RECOVER = [M.quiet(90000)]   # after a frame that was damaged on purpose: longer than the default waiting time of 65536 cycles, so that
                             # a decoder still waiting for an answer is searching again when the next request comes


def relabel(burst, defect):
    return burst._replace(sent=burst.sent._replace(defect=defect))


# ---- NFC-A pieces (ISO/IEC 14443-3 / -4 commands: only the bytes a decoder's protocol tracking looks at matter)
def reqa(cmd=0x26, answer=True, **kw):
    return [M.nfca_poll(bytes([cmd]), bits7=True, **kw)] + ([M.nfca_listen(b"\x44\x03", crc=False)] if answer else [])


def select():
    uid = b"\x88\x04\x5a\x1c"
    bcc = bytes([uid[0] ^ uid[1] ^ uid[2] ^ uid[3]])
    return [M.nfca_poll(b"\x93\x20", crc=False), M.nfca_listen(uid + bcc, crc=False),
            M.nfca_poll(b"\x93\x70" + uid + bcc), M.nfca_listen(b"\x20")]


def rats(fsdi=8, tb=None, ats_kw=None):
    """RATS with that FSDI; ATS with TA and TC, and with TB = `tb` (FWI in its high nibble) unless tb is None"""
    t0 = 0x50 | (0x20 if tb is not None else 0) | 0x08
    body = bytes([t0, 0x77]) + (bytes([tb]) if tb is not None else b"") + b"\x02" + b"\x80\x31"
    return [M.nfca_poll(bytes([0xE0, fsdi << 4])), M.nfca_listen(bytes([len(body) + 1]) + body, **(ats_kw or {}))]


def iblock(n, rate=106, pcb=0x02, answer=True, poll_kw=None, listen_kw=None):
    out = [M.nfca_poll(bytes([pcb]) + PAY[:n], rate=rate, **(poll_kw or {}))]
    if answer:
        out.append(M.nfca_listen(bytes([pcb]) + PAY[300:300 + n], rate=rate, **(listen_kw or {})))
    return out


def waiting_window(fwi, tb_present=True, outside=True):
    """an ATS that sets the frame waiting time to 4096 << fwi carrier cycles, then an I-block answered just inside it and (unless
    not outside) one answered just after it (the reader has given up: no answer is to be reported)"""
    eff = 4 if (fwi == 15 or not tb_present) else fwi
    fwt = 4096 << eff
    out = reqa() + rats(8, tb=(fwi << 4) | 1 if tb_present else None)
    out += iblock(12, listen_kw={"gap": max(1200, fwt - 700)})
    if outside:
        out += [M.nfca_poll(b"\x03" + PAY[:12]), relabel(M.nfca_listen(b"\x03" + PAY[312:324], gap=fwt + 700), "late")]
        out += RECOVER + iblock(5)
    return out


# ---- NFC-B pieces
def unheard(items):
    """After an NFC-B answer that breaks off, the reference reports nothing more to the end of the stream, neither frames nor the
    carrier going: its answer decoder waits for the end of the frame without a time limit. What is sent after one is listed as
    unheard (no frame is expected), and is there for the comparisons with the reference: the kernels must stay as deaf."""
    return [relabel(it, "unheard") if isinstance(it, M.Burst) else it for it in items]



def reqb(fsdi=8, fwi=4, rate=106, answer=True, atqb_kw=None, **kw):
    atqb = b"\x50" + b"\x12\x34\x56\x78" + b"\x00\x00\x00\x00" + bytes([0x00, (fsdi << 4) | 1, (fwi << 4)])
    return [M.nfcb_poll(b"\x05\x00\x00", rate=rate, **kw)] + ([M.nfcb_listen(atqb, rate=rate, **(atqb_kw or {}))] if answer else [])


def attrib(fsdi=8, tr0=0, rate=106, answer=True):
    cmd = b"\x1d" + b"\x12\x34\x56\x78" + bytes([tr0 << 6, fsdi, 0x01, 0x00])
    return [M.nfcb_poll(cmd, rate=rate)] + ([M.nfcb_listen(b"\x00", rate=rate)] if answer else [])


def bblock(n, rate=106, answer=True, poll_kw=None, listen_kw=None):
    return [M.nfcb_poll(b"\x02" + PAY[:n], rate=rate, **(poll_kw or {}))] + \
           ([M.nfcb_listen(b"\x02" + PAY[300:300 + n], rate=rate, **(listen_kw or {}))] if answer else [])


# ---- NFC-F pieces
def reqc(rate=212, rev=False, tsn=0, answer=True, listen_kw=None, **kw):
    out = [M.nfcf_poll(bytes([0x00, 0xFF, 0xFF, 0x01, tsn]), rate=rate, reversed_polarity=rev, **kw)]
    if answer:
        out.append(M.nfcf_listen(b"\x01" + PAY[:16], rate=rate, reversed_polarity=rev, **(listen_kw or {})))
    return out


def fblock(n, rate=212, rev=False, answer=True, poll_kw=None, listen_kw=None):
    out = [M.nfcf_poll(b"\x06" + PAY[:n - 1], rate=rate, reversed_polarity=rev, **(poll_kw or {}))]
    if answer:
        out.append(M.nfcf_listen(b"\x07" + PAY[300:300 + n - 1], rate=rate, reversed_polarity=rev, **(listen_kw or {})))
    return out


# ---- NFC-V pieces
def vblock(n_req, n_ans, mode=4, answer=True, poll_kw=None, listen_kw=None):
    out = [M.nfcv_poll(b"\x02\x21" + PAY[:n_req], mode=mode, **(poll_kw or {}))]
    if answer:
        out.append(M.nfcv_listen(b"\x00" + PAY[300:300 + n_ans], **(listen_kw or {})))
    return out


def mixed(a_answers=True):
    return (reqa(answer=a_answers) + iblock(20, answer=a_answers) + [M.carrier_off(30000)] + reqb() + attrib() + bblock(20) + [M.quiet(40000)] + reqc() + fblock(20)
            + [M.carrier_off(50000), M.quiet(30000)] + vblock(2, 12) + [M.quiet(30000)] + reqa(0x52, answer=a_answers) + iblock(9, answer=a_answers))


# the weak-signal sweeps: depth of the reader's modulation and load of the card's, from clearly decodable down to nothing, the
# steps crowded where a plain run of the reference loses the frames (found by trying; nothing here depends on where exactly)
WEAK = {
    "a": ((0.95, 0.90, 0.87, 0.85, 0.83, 0.80, 0.60), (0.2, 0.05, 0.03, 0.025, 0.02, 0.015, 0.005)),
    "b": ((0.50, 0.20, 0.15, 0.13, 0.11, 0.10, 0.05), (0.25, 0.03, 0.01, 0.008, 0.006, 0.005, 0.002)),
    "f": ((0.45, 0.30, 0.27, 0.24, 0.22, 0.20, 0.10), (0.25, 0.03, 0.01, 0.008, 0.006, 0.004, 0.002)),
    "v": ((0.97, 0.90, 0.87, 0.85, 0.83, 0.80, 0.50), (0.2, 0.05, 0.03, 0.025, 0.02, 0.015, 0.005)),
}


def _table():
    t = []

    def add(name, group, items, fs=FS, where="all", **kw):
        t.append(Case(name, group, fs, items, kw, where))

    # ---- 1: every technology, rate and direction, short and long
    for rate in (106, 212, 424):
        add("a%d short and long" % rate, 1, lambda rate=rate: reqa() + rats(8) + iblock(8, rate) + iblock(60, rate) + iblock(250, rate), seed=11 + rate)
    add("b106 short and long", 1, lambda: reqb() + attrib() + bblock(8) + bblock(250), seed=21)
    add("b212 polls short and long", 1, lambda: reqb(rate=212, answer=False) + RECOVER + attrib(rate=212, answer=False)
        + RECOVER + bblock(250, 212, answer=False), seed=22)
    add("b212 with answers", 1, lambda: reqb(rate=212) + attrib(rate=212) + bblock(40, 212), seed=23)
    add("b424", 1, lambda: reqb(rate=424) + attrib(rate=424) + bblock(40, 424), seed=24)
    # (NFC-F: a length byte of 251 gives 2 sync bytes + 253 = 255 bytes; one byte more fills the 256 bytes that the reference allows a
    # frame after REQC and is flagged Truncated; the frame with length byte 255 comes last and is listed as oversize)
    for rate in (212, 424):
        for rev in (False, True):
            add("f%d %s short and long" % (rate, "reversed" if rev else "observed"), 1,
                lambda rate=rate, rev=rev: reqc(rate, rev) + fblock(20, rate, rev) + fblock(250, rate, rev)
                + [relabel(fblock(254, rate, rev, answer=False)[0], "oversize")], seed=30 + rate + rev)
    add("v 1-of-4 short and long", 1, lambda: vblock(1, 8) + vblock(64, 100), seed=41)
    add("v 1-of-256", 1, lambda: vblock(1, 70, mode=256), seed=42)

    # ---- 2: defects
    add("a106 wrong crc", 2, lambda: reqa() + rats(8) + iblock(17, poll_kw={"bad_crc": True}) + iblock(17, listen_kw={"bad_crc": True}) + iblock(4), seed=50)
    add("a106 wrong parity", 2, lambda: reqa() + rats(8) + iblock(30, poll_kw={"bad_parity": 9}) + iblock(30, listen_kw={"bad_parity": 17}) + iblock(4), seed=51)
    add("a424 wrong crc and parity", 2, lambda: reqa() + rats(8) + iblock(30, 424, poll_kw={"bad_parity": 9}) + iblock(30, 424, listen_kw={"bad_parity": 17})
        + iblock(11, 424, listen_kw={"bad_crc": True}) + iblock(4, 424), seed=52)
    add("a212 wrong last parity", 2, lambda: reqa() + rats(8) + iblock(12, 212, listen_kw={"bad_parity": 14}) + iblock(4, 212), seed=53)
    add("a106 truncated", 2, lambda: reqa() + rats(8) + iblock(40, poll_kw={"cut": 200}, answer=False) + RECOVER + iblock(40, listen_kw={"cut": 201}) + RECOVER
        + iblock(40, listen_kw={"cut": 150, "cut_mode": "off"}) + RECOVER + reqa() + iblock(40, listen_kw={"cut": 100, "cut_mode": "end"}), seed=54)
    add("a212 truncated", 2, lambda: reqa() + rats(8) + iblock(40, 212, poll_kw={"cut": 200}, answer=False) + RECOVER + iblock(40, 212, listen_kw={"cut": 201})
        + RECOVER + iblock(6, 212), seed=55)
    add("a106 answers absent, early and late", 2, lambda: reqa() + [M.nfca_poll(b"\x26", bits7=True)] + RECOVER
        + [M.nfca_poll(b"\x52", bits7=True), relabel(M.nfca_listen(b"\x44\x03", crc=False, gap=300), "early")] + RECOVER
        + [M.nfca_poll(b"\x52", bits7=True), relabel(M.nfca_listen(b"\x44\x03", crc=False, gap=4000), "late")] + RECOVER
        + reqa() + rats(8) + iblock(10, answer=False) + RECOVER + [M.nfca_poll(b"\x03" + PAY[:10]), relabel(M.nfca_listen(b"\x03" + PAY[300:310], gap=70000), "late")]
        + RECOVER + iblock(10), seed=56)
    add("b106 wrong crc", 2, lambda: reqb() + attrib() + bblock(17, poll_kw={"bad_crc": True}) + bblock(17, listen_kw={"bad_crc": True}) + bblock(4), seed=60)
    add("b106 truncated", 2, lambda: reqb() + attrib() + bblock(40, poll_kw={"cut": 200}, answer=False) + RECOVER + bblock(40, listen_kw={"cut": 201}) + RECOVER
        + unheard(reqb() + bblock(5) + [M.quiet(30000), M.carrier_off(40000), M.quiet(30000)] + reqa() + reqb()), seed=61)
    add("b106 answer breaks off with the carrier", 2, lambda: reqb() + bblock(40, listen_kw={"cut": 150, "cut_mode": "off"}) + RECOVER + unheard(reqb() + bblock(5)), seed=64)
    add("b106 stream ends in an answer", 2, lambda: reqb() + bblock(40, listen_kw={"cut": 100, "cut_mode": "end"}), seed=65)
    add("b212 wrong crc and truncated polls", 2, lambda: reqb(rate=212, answer=False) + RECOVER + bblock(17, 212, answer=False, poll_kw={"bad_crc": True}) + RECOVER
        + bblock(40, 212, answer=False, poll_kw={"cut": 200}) + RECOVER + bblock(9, 212, answer=False), seed=62)
    add("b106 answers absent, early and late", 2, lambda: reqb() + reqb(answer=False) + RECOVER
        + [M.nfcb_poll(b"\x05\x00\x08"), relabel(reqb(atqb_kw={"gap": 300})[1], "early")] + RECOVER
        + [M.nfcb_poll(b"\x05\x00\x08"), relabel(reqb(atqb_kw={"gap": 9500})[1], "late")] + RECOVER + reqb() + attrib() + bblock(10), seed=63)
    for rate in (212, 424):
        add("f%d wrong crc and sync" % rate, 2, lambda rate=rate: reqc(rate) + fblock(17, rate, poll_kw={"bad_crc": True}) + fblock(17, rate, listen_kw={"bad_crc": True})
            + fblock(9, rate, poll_kw={"sync": b"\xB2\x4C"}) + fblock(9, rate, listen_kw={"sync": b"\xB3\x4D"}) + fblock(4, rate), seed=70 + rate)
        add("f%d truncated" % rate, 2, lambda rate=rate: reqc(rate) + fblock(40, rate, poll_kw={"cut": 200}, answer=False) + RECOVER + fblock(40, rate, listen_kw={"cut": 201})
            + RECOVER + fblock(40, rate, True, listen_kw={"cut": 150, "cut_mode": "off"}) + RECOVER + reqc(rate) + fblock(40, rate, listen_kw={"cut": 180, "cut_mode": "end"}), seed=72 + rate)
    add("f212 answers absent, early and late", 2, lambda: reqc() + reqc(answer=False) + RECOVER
        + [reqc()[0], relabel(reqc(listen_kw={"gap": 400})[1], "early")] + RECOVER + [reqc()[0], relabel(reqc(listen_kw={"gap": 52000})[1], "late")] + RECOVER
        + reqc() + fblock(10), seed=74)
    add("v wrong crc", 2, lambda: vblock(3, 9, poll_kw={"bad_crc": True}) + vblock(3, 9, listen_kw={"bad_crc": True}) + vblock(1, 4), seed=80)
    add("v truncated", 2, lambda: vblock(8, 0, poll_kw={"cut": 20}, answer=False) + RECOVER + vblock(2, 30, listen_kw={"cut": 100})
        + RECOVER + vblock(2, 30, listen_kw={"cut": 77, "cut_mode": "off"}) + RECOVER + vblock(2, 30, listen_kw={"cut": 60, "cut_mode": "end"}), seed=81)
    # (the early answer begins right behind the request: its subcarrier starts 768 cycles later, inside the guard time of 1024. The
    # reference decodes it all the same - the start pattern it looks for ends after the guard time - so it is listed as sent whole)
    add("v answers absent, early and late", 2, lambda: vblock(2, 6) + vblock(2, 6, answer=False) + RECOVER
        + vblock(2, 6, listen_kw={"gap": 0}) + RECOVER
        + [vblock(2, 6)[0], relabel(vblock(2, 6, listen_kw={"gap": 400000})[1], "late")] + RECOVER + vblock(2, 6), seed=82)

    # ---- 3: protocol feedback
    add("a106 select, halt, wake up", 3, lambda: reqa() + select() + [M.nfca_poll(b"\x50\x00")] + [M.quiet(20000)] + reqa(0x52) + select() + rats(8) + iblock(9), seed=90)
    for fsdi, size in ((0, 16), (5, 64), (8, 256)):
        add("a106 rats fsdi %d then frames over %d bytes" % (fsdi, size), 3,
            lambda fsdi=fsdi, size=size: reqa() + rats(fsdi) + [M.nfca_poll(b"\x02" + PAY[:8]), relabel(M.nfca_listen(b"\x02" + PAY[300:300 + size + 5]), "oversize")]
            + RECOVER + iblock(6) + reqa() + rats(fsdi) + iblock(size - 3 - 6), seed=91 + fsdi)
    add("a424 rats fsdi 5 then a frame over 64 bytes", 3, lambda: reqa() + rats(5) + [M.nfca_poll(b"\x02" + PAY[:8], rate=424),
        relabel(M.nfca_listen(b"\x02" + PAY[300:380], rate=424), "oversize")] + RECOVER + iblock(6, 424), seed=99)
    add("a106 ats without tb", 3, lambda: waiting_window(0, tb_present=False), seed=100)
    for fwi in (0, 4, 15):
        add("a106 ats fwi %d" % fwi, 3, lambda fwi=fwi: waiting_window(fwi), seed=101 + fwi)
    add("a106 ats fwi 8", 3, lambda: waiting_window(8), seed=109, where="step")
    # (4096 << 14 carrier cycles are 49.5 M samples: the answer comes well inside the window after 10 M cycles and the stream ends at
    # 2^23 samples; "just outside" is not tested for FWI 14)
    add("a106 ats fwi 14", 3, lambda: reqa() + rats(8, tb=0xE1) + iblock(12, listen_kw={"gap": 10000000}), seed=115, where="device", max_samples=1 << 23)
    add("a106 pps then 212", 3, lambda: reqa() + select() + rats(8) + [M.nfca_poll(b"\xD0\x11\x05"), M.nfca_listen(b"\xD0")] + iblock(30, 212) + iblock(7, 212), seed=120)
    # (the reference flags the card's nonce, the first frame after AUTH, as Encrypted already)
    add("a106 mifare auth then ciphered frames", 3, lambda: reqa() + select() + [M.nfca_poll(b"\x60\x04"), relabel(M.nfca_listen(PAY[:4], crc=False), "ciphered")]
        + [relabel(M.nfca_poll(PAY[4:12], crc=False, bad_parity=3), "ciphered"), relabel(M.nfca_listen(PAY[12:16], crc=False, bad_parity=1), "ciphered")]
        + [relabel(M.nfca_poll(PAY[20:24], crc=False, bad_parity=0), "ciphered"), relabel(M.nfca_listen(PAY[30:48], crc=False, bad_parity=5), "ciphered")]
        + [relabel(M.nfca_poll(PAY[50:54], crc=False), "ciphered"), relabel(M.nfca_listen(b"\x0A", bits7=True), "ciphered")], seed=121)
    # (NFC-B: TR1 of 1280 cycles and the start of frame of 1536 have to be over inside the waiting time)
    for fsdi, fwi in ((0, 0), (5, 4), (8, 7)):
        fwt = 4096 << fwi
        add("b106 atqb fsdi %d fwi %d" % (fsdi, fwi), 3, lambda fsdi=fsdi, fwi=fwi, fwt=fwt: reqb(fsdi, fwi)
            + [M.nfcb_poll(b"\x02" + PAY[:5]), relabel(M.nfcb_listen(b"\x02" + PAY[300:300 + (16, 64, 256)[(0, 5, 8).index(fsdi)] + 5], gap=1200), "oversize")]
            + RECOVER + bblock(5, listen_kw={"gap": max(1200, fwt - 4000)}) + [M.quiet(20000)]
            + [M.nfcb_poll(b"\x03" + PAY[:5]), relabel(M.nfcb_listen(b"\x03" + PAY[300:305], gap=fwt + 700), "late")] + RECOVER + bblock(6, listen_kw={"gap": 1200}), seed=130 + fsdi)
    # (ATTRIB: TR0 code 0, 1 and 2 ask for 1024, 768 and 256 cycles of silence before the answer: an answer after 500 cycles is
    # early for code 0, one after 800 or 500 cycles is in time for codes 1 and 2)
    for tr0, fsdi in ((0, 2), (1, 8), (2, 5)):
        add("b106 attrib tr0 %d fsdi %d" % (tr0, fsdi), 3, lambda tr0=tr0, fsdi=fsdi: reqb() + attrib(fsdi, tr0) + bblock(9, listen_kw={"gap": 1100})
            + [bblock(9)[0], bblock(9, listen_kw={"gap": (500, 800, 500)[tr0]})[1] if tr0 else relabel(bblock(9, listen_kw={"gap": 500})[1], "early")] + RECOVER
            + [M.nfcb_poll(b"\x02" + PAY[:5]), relabel(M.nfcb_listen(b"\x02" + PAY[300:300 + (32, 256, 64)[tr0] + 5]), "oversize")] + RECOVER + bblock(6), seed=140 + tr0)
    # (NFC-F: the preamble of 48 bits has to be over inside the window of 512 * 64 + (TSN + 1) * 256 * 64 cycles)
    for tsn in (0, 3):
        window = 512 * 64 + (tsn + 1) * 256 * 64
        add("f212 reqc with %d slots" % (tsn + 1), 3, lambda tsn=tsn, window=window: reqc(tsn=tsn, listen_kw={"gap": window - 5000})
            + [reqc(tsn=tsn)[0], relabel(reqc(listen_kw={"gap": window + 700})[1], "late")] + RECOVER + reqc(tsn=tsn) + fblock(12), seed=150 + tsn)
    add("f424 reqc with 2 slots", 3, lambda: reqc(424, tsn=1, listen_kw={"gap": 512 * 64 + 2 * 256 * 64 - 5000}) + fblock(12, 424, listen_kw={"gap": 60000}), seed=155)

    # ---- 4: technologies after one another
    add("a b f v a with carrier gaps", 4, mixed, seed=160)
    add("f424 v a212 b", 4, lambda: reqc(424, True) + fblock(30, 424, True) + [M.quiet(30000)] + vblock(2, 20, mode=256) + [M.carrier_off(20000), M.quiet(30000)]
        + reqa() + iblock(30, 212) + [M.quiet(30000)] + reqb(5, 2) + attrib(5) + bblock(30), seed=161)

    # ---- 5: weak signals: a weak request with a plain answer, then a plain request with a weak answer
    for k in range(7):
        d, l = WEAK["a"][0][k], WEAK["a"][1][k]
        add("weak a106 step %d" % k, 5, lambda d=d, l=l: reqa(depth=d) + iblock(20, poll_kw={"depth": d}) + RECOVER
            + [reqa()[0], M.nfca_listen(b"\x44\x03", crc=False, load=l)] + iblock(20, listen_kw={"load": l}), seed=200 + k)
        add("weak a424 step %d" % k, 5, lambda d=d, l=l: reqa() + iblock(20, 424, poll_kw={"depth": d}) + RECOVER + iblock(20, 424, listen_kw={"load": l}), seed=210 + k)
        d, l = WEAK["b"][0][k], WEAK["b"][1][k]
        add("weak b106 step %d" % k, 5, lambda d=d, l=l: reqb(depth=d) + bblock(20, poll_kw={"depth": d}) + RECOVER
            + reqb(atqb_kw={"load": l}) + bblock(20, listen_kw={"load": l}), seed=220 + k)
        d, l = WEAK["f"][0][k], WEAK["f"][1][k]
        for rate in (212, 424):
            add("weak f%d step %d" % (rate, k), 5, lambda d=d, l=l, rate=rate: reqc(rate, depth=d) + fblock(20, rate, poll_kw={"depth": d}) + RECOVER
                + reqc(rate, listen_kw={"depth": l}) + fblock(20, rate, listen_kw={"depth": l}), seed=230 + k + rate)
        d, l = WEAK["v"][0][k], WEAK["v"][1][k]
        add("weak v step %d" % k, 5, lambda d=d, l=l: vblock(2, 10, poll_kw={"depth": d}) + RECOVER + vblock(2, 10, listen_kw={"load": l}), seed=250 + k)

    # (with this seed the reference loses the first answer at 424 kbps although nothing is weak: the threshold of its BPSK start search
    # is the deviation it meets at the end of the guard time, noise included. Kept for that, and exempt like the sweeps.)
    add("weak a424 plain answer lost with seed 434", 5, lambda: reqa() + rats(8) + iblock(8, 424) + iblock(60, 424) + iblock(250, 424), seed=434)

    # ---- 6: groups 1-4 at 5 and 2.5 MS/s, a representative per technology. At 2.5 MS/s the NFC-A scenarios send requests alone
    # (one scenario with answers is kept: tests/test_modulated.py lists it as an exception)
    for fs in (5000000, 2500000):
        tag = " at %g MS/s" % (fs / 1e6)
        ans = fs != 2500000
        add("a106 short and long" + tag, 6, lambda ans=ans: reqa(answer=ans) + (rats(8) if ans else RECOVER) + iblock(8, answer=ans) + iblock(250, answer=ans), fs=fs, seed=300)
        if ans:
            add("a106 defects" + tag, 6, lambda: reqa() + rats(8) + iblock(17, listen_kw={"bad_crc": True}) + iblock(30, listen_kw={"bad_parity": 17})
                + iblock(40, listen_kw={"cut": 201}) + RECOVER + iblock(4), fs=fs, seed=301)
            add("a106 ats fwi 0" + tag, 6, lambda: waiting_window(0), fs=fs, seed=302)
        else:
            add("a106 defects in requests" + tag, 6, lambda: reqa(answer=False) + iblock(17, answer=False, poll_kw={"bad_crc": True}) + iblock(30, answer=False, poll_kw={"bad_parity": 17})
                + iblock(40, answer=False, poll_kw={"cut": 201}) + RECOVER + iblock(4, answer=False), fs=fs, seed=301)
            add("a106 with answers" + tag, 6, lambda: reqa() + rats(8) + iblock(8) + iblock(40), fs=fs, seed=302)
        add("b106 short and long" + tag, 6, lambda: reqb() + attrib() + bblock(8) + bblock(250), fs=fs, seed=303)
        add("b106 defects" + tag, 6, lambda: reqb() + attrib() + bblock(17, listen_kw={"bad_crc": True}) + bblock(40, listen_kw={"cut": 201}) + RECOVER + unheard(bblock(4)), fs=fs, seed=304)
        add("b106 atqb fsdi 5 fwi 4" + tag, 6, lambda: reqb(5, 4) + bblock(5, listen_kw={"gap": 65536 - 4000}) + [M.quiet(20000)]
            + [M.nfcb_poll(b"\x03" + PAY[:5]), relabel(M.nfcb_listen(b"\x03" + PAY[300:305], gap=65536 + 700), "late")] + RECOVER + bblock(6), fs=fs, seed=305)
        add("f212 short and long" + tag, 6, lambda: reqc() + fblock(20) + fblock(250), fs=fs, seed=306)
        add("f212 defects" + tag, 6, lambda: reqc() + fblock(17, listen_kw={"bad_crc": True}) + fblock(40, listen_kw={"cut": 201}) + RECOVER + fblock(4), fs=fs, seed=307)
        add("f212 reqc with 4 slots" + tag, 6, lambda: reqc(tsn=3, listen_kw={"gap": 512 * 64 + 4 * 256 * 64 - 5000}) + fblock(12), fs=fs, seed=308)
        add("v short and long" + tag, 6, lambda: vblock(1, 8) + vblock(64, 100), fs=fs, seed=309)
        add("v defects" + tag, 6, lambda: vblock(3, 9, listen_kw={"bad_crc": True}) + vblock(2, 30, listen_kw={"cut": 100}) + RECOVER + vblock(1, 4), fs=fs, seed=310)
        add("a b f v a with carrier gaps" + tag, 6, lambda ans=ans: mixed(ans), fs=fs, seed=311)
    return t


CASES = _table()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def build(case, grid=False):
    """(float32 samples, [Sent]) of a scenario; grid: rounded onto the int16 grid of a capture"""
    if isinstance(case, str):
        case = BY_NAME[case]
    return M.exchange(case.items(), fs=case.fs, grid=grid, **case.kw)
